// The export stages' order-preserving compaction, stated once: RemovePoints (io/points_batch.cc:22-49) on the device
// (DESIGN.md sections 3.10, 3.13, 3.14).  A stage's kernel writes a keep flag a point and the largest squared norm of the
// kept ones; scan_kept, read_kept (ONE read-back) and emit_kept make the cloud of the survivors (internal.h).  What a stage
// does between the steps, and what it makes of "nothing kept", is the stage's.
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>

#include "device_common.h"

namespace dliom {
namespace {

constexpr int kBlock = 256;

// the largest squared norm of the kept points (cloud_max_norm's order), for the compacted cloud's bound
__global__ __launch_bounds__(kBlock) void kept_max_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ z, const unsigned* __restrict__ keep, unsigned n,
                                                          unsigned* __restrict__ max_sq) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  note_kept(i < n && keep[i] != 0u ? norm_word(x[i], y[i], z[i]) : 0u, max_sq);
}

// RemovePoints (points_batch.cc:22-49): the survivors in input order, and their input indices
__global__ __launch_bounds__(kBlock) void scatter_kept_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                              const float* __restrict__ z, unsigned n,
                                                              const unsigned* __restrict__ keep, const unsigned* __restrict__ inclusive,
                                                              float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ oz,
                                                              int* __restrict__ index) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || keep[i] == 0u) return;
  const unsigned at = inclusive[i] - 1u;
  ox[at] = x[i];
  oy[at] = y[i];
  oz[at] = z[i];
  index[at] = static_cast<int>(i);
}

// The survivors' intensities and colours, by the input indices the scatter has just left in scratch
__global__ __launch_bounds__(kBlock) void gather_attributes_kernel(const int* __restrict__ index, unsigned kept,
                                                                   const float* __restrict__ src_i, const float* __restrict__ src_c,
                                                                   float* __restrict__ dst_i, float* __restrict__ dst_c) {
  const unsigned j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= kept) return;
  const size_t i = static_cast<size_t>(index[j]);
  if (src_i != nullptr) dst_i[j] = src_i[i];
  if (src_c != nullptr) {
    dst_c[3 * static_cast<size_t>(j)] = src_c[3 * i];
    dst_c[3 * static_cast<size_t>(j) + 1] = src_c[3 * i + 1];
    dst_c[3 * static_cast<size_t>(j) + 2] = src_c[3 * i + 2];
  }
}

}  // namespace

int AttrBlock::alloc(dliom_ctx* ctx, size_t count) {
  if (count == 0) return DLIOM_OK;
  DLIOM_TRY(device_block_alloc(ctx->device, 4 * count, &base, &bytes));
  p = static_cast<float*>(base);
  return DLIOM_OK;
}
void AttrBlock::release(dliom_ctx* ctx) {
  if (base != nullptr) device_block_free(ctx->device, base, bytes);
  base = nullptr;
  bytes = 0;
  p = nullptr;
}

int carve_compact(dliom_ctx* ctx, int64_t n, CompactScratch* s, size_t extra_bytes, size_t zeroed_extra_bytes) {
  size_t tmp = 0;
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tmp, static_cast<const unsigned*>(nullptr), static_cast<unsigned*>(nullptr),
                                                 static_cast<int>(n), ctx->stream));
  const size_t per = align256(4 * static_cast<size_t>(n));
  DLIOM_TRY(ctx->outlier.reserve(3 * per + 256 + align256(tmp) + extra_bytes));
  char* b = static_cast<char*>(ctx->outlier.p);
  s->keep = reinterpret_cast<unsigned*>(b);
  s->inclusive = reinterpret_cast<unsigned*>(b + per);
  s->index = reinterpret_cast<int*>(b + 2 * per);
  s->max_sq = reinterpret_cast<unsigned*>(b + 3 * per);
  s->tmp = b + 3 * per + 256;
  s->tmp_bytes = tmp;
  s->extra = b + 3 * per + 256 + align256(tmp);
  const FillJob fills[2] = {{s->max_sq, 4, 0u}, {s->extra, zeroed_extra_bytes, 0u}};
  return fill_multi(ctx, fills, zeroed_extra_bytes > 0 ? 2 : 1);
}

int empty_cloud(dliom_ctx* ctx, dliom_cloud** out) {
  float *x, *y, *z;
  DLIOM_TRY(alloc_device_cloud(ctx, 0, out, &x, &y, &z));
  return finish_device_cloud(ctx, *out, 0.f);
}

int max_of_kept(dliom_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, const CompactScratch& s) {
  hipLaunchKernelGGL(kept_max_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, ctx->stream, x, y, z, s.keep, static_cast<unsigned>(n), s.max_sq);
  return hipGetLastError() == hipSuccess ? DLIOM_OK : DLIOM_ERR_HIP;
}

int scan_kept(dliom_ctx* ctx, int64_t n, const CompactScratch& s) {
  size_t tmp = s.tmp_bytes;
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(s.tmp, tmp, s.keep, s.inclusive, static_cast<int>(n), ctx->stream));
  return DLIOM_OK;
}

int read_kept(dliom_ctx* ctx, int64_t n, const CompactScratch& s, const GatherJob* more, int64_t* kept, float* max_sq,
              unsigned* more_host) {
  unsigned* host = pinned_at<unsigned>(ctx, kPinReadback);
  GatherJob jobs[3] = {{s.inclusive + (n - 1), 1}, {s.max_sq, 1}, {}};
  if (more != nullptr) jobs[2] = *more;
  DLIOM_TRY(gather_and_wait(ctx, jobs, more != nullptr ? 3 : 2, host));
  *kept = host[0];
  std::memcpy(max_sq, &host[1], 4);
  if (more != nullptr) std::memcpy(more_host, host + 2, 4 * static_cast<size_t>(more->words));
  return DLIOM_OK;
}

int emit_kept(dliom_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, const CompactScratch& s, int64_t kept,
              float max_sq, dliom_cloud** out, int32_t* kept_index) {
  float *ox, *oy, *oz;
  DLIOM_TRY(alloc_device_cloud(ctx, kept, out, &ox, &oy, &oz));
  hipLaunchKernelGGL(scatter_kept_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, ctx->stream, x, y, z, static_cast<unsigned>(n), s.keep,
                     s.inclusive, ox, oy, oz, s.index);
  int st = hipGetLastError() == hipSuccess ? DLIOM_OK : DLIOM_ERR_HIP;
  if (st == DLIOM_OK) st = finish_device_cloud(ctx, *out, std::sqrt(max_sq));  // sqrt is monotone: the max of the norms
  if (st == DLIOM_OK && kept_index != nullptr) {
    if (hipMemcpyAsync(kept_index, s.index, static_cast<size_t>(kept) * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
      st = DLIOM_ERR_HIP;
    ++ctx->host_syncs;
  }
  if (st != DLIOM_OK) {
    dliom_cloud_destroy(*out);
    *out = nullptr;
  }
  return st;
}

int compact_kept(dliom_ctx* ctx, const dliom_cloud* in, const CompactScratch& s, const unsigned* flag_word, unsigned* flag,
                 dliom_cloud** out, int32_t* kept_index, int64_t capacity, int64_t* num_kept) {
  DLIOM_TRY(scan_kept(ctx, in->n, s));
  const GatherJob flag_job{flag_word, 1};
  int64_t kept;
  float max_sq;
  DLIOM_TRY(read_kept(ctx, in->n, s, flag_word != nullptr ? &flag_job : nullptr, &kept, &max_sq, flag));
  if (flag_word != nullptr && *flag != 0u) return DLIOM_OK;  // the caller refuses
  *num_kept = kept;
  if (kept_index != nullptr && capacity < kept) return DLIOM_ERR_CAPACITY;
  if (kept == 0) return empty_cloud(ctx, out);
  return emit_kept(ctx, in->d_x, in->d_y, in->d_z, in->n, s, kept, max_sq, out, kept_index);
}

int gather_batch_attributes(dliom_ctx* ctx, const int* d_index, int64_t kept, const float* src_intensities, const float* src_colors,
                            float* dst_intensities, float* dst_colors) {
  if (kept <= 0 || (src_intensities == nullptr && src_colors == nullptr)) return DLIOM_OK;
  hipLaunchKernelGGL(gather_attributes_kernel, dim3(blocks_of(kept, kBlock)), dim3(kBlock), 0, ctx->stream, d_index, static_cast<unsigned>(kept),
                     src_intensities, src_colors, dst_intensities, dst_colors);
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

int compact_batch(dliom_points_batch* b, const CompactScratch& s, const unsigned* flag_word, unsigned* flag, int64_t* num_kept) {
  dliom_ctx* ctx = b->ctx;
  dliom_cloud* kept_cloud = nullptr;
  int64_t kept = 0;
  DLIOM_TRY(compact_kept(ctx, b->cloud, s, flag_word, flag, &kept_cloud, nullptr, 0, &kept));
  if (kept_cloud == nullptr) return DLIOM_OK;  // the flag is set: nothing was compacted
  // s.index holds the survivors' input indices until the next stage carves the scratch
  AttrBlock ki, kc;
  int st = DLIOM_OK;
  if (b->intensities.p != nullptr) st = ki.alloc(ctx, static_cast<size_t>(kept));
  if (st == DLIOM_OK && b->colors.p != nullptr) st = kc.alloc(ctx, 3 * static_cast<size_t>(kept));
  if (st == DLIOM_OK) st = gather_batch_attributes(ctx, s.index, kept, ki.p != nullptr ? b->intensities.p : nullptr,
                                                   kc.p != nullptr ? b->colors.p : nullptr, ki.p, kc.p);
  if (st != DLIOM_OK) {
    ki.release(ctx);
    kc.release(ctx);
    dliom_cloud_destroy(kept_cloud);
    return st;
  }
  dliom_cloud_destroy(b->cloud);  // (waits for the device: the gather has read the old arrays)
  b->intensities.release(ctx);
  b->colors.release(ctx);
  b->cloud = kept_cloud;
  b->intensities = ki;
  b->colors = kc;
  if (kept == 0) b->single_color = false;  // RemovePoints leaves empty vectors: an empty batch has no attributes
  *num_kept = kept;
  return DLIOM_OK;
}

}  // namespace dliom
