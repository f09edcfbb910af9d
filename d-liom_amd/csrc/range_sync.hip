// The RangeDataSynchronizer's per-point work on device objects (dliom.h "Two range sensors' clouds merged on the device",
// DESIGN.md section 3.21): StampRangeData and the merge of a secondary lidar's overlapping part into the prior lidar's
// cloud (mapping/internal/3d/range_data_synchronizer.cc:29-130), in the order libstdc++'s std::sort leaves the merged
// records in -- equal times included, through rotational_histogram.hip's replay (std_sort_order_enqueue).
//
// Nothing is materialised but the merged times: the sort takes those as its keys, and the gather behind it reads a merged
// record straight from the object it came from (index < n_primary: the prior cloud's; else the secondary's, re-based).
// The keys and the call's words live in ctx->outlier, the sort works in ctx->misc.  Two read-backs: the overlap's bounds
// (the sort's launches take the merged size from the host), then the sort's status with the first and the last t.
#include <cstring>

#include "device_common.h"
#include "timed_cloud.h"

namespace dliom {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxMerged = 1 << 22;  // std_sort_order_enqueue's limit
enum { kWordStart = 0, kWordEnd = 1, kWordFront = 2, kWordBack = 3, kWords = 4 };

// t_i = float(-scan_period + i * duration) in double, the product rounded on its own; the last t = 0
__global__ __launch_bounds__(kBlock) void stamp_kernel(const float4* __restrict__ in, uint32_t n, double scan_period, double duration,
                                                       float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float4 v = in[i];
  v.w = i + 1u == n ? 0.f : __double2float_rn(__dadd_rn(-scan_period, __dmul_rn(static_cast<double>(i), duration)));
  out[i] = v;
}

// words[kWordStart] (n on entry) = the first i with current_start <= st + double(t_i) <= current_end
__global__ __launch_bounds__(kBlock) void overlap_start_kernel(const float4* __restrict__ sec, uint32_t n, double st, double current_start,
                                                               double current_end, unsigned* __restrict__ words) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double t = __dadd_rn(st, static_cast<double>(sec[i].w));
  if (t >= current_start && t <= current_end) atomicMin(&words[kWordStart], i);
}

// words[kWordEnd] (n on entry) = the first i behind words[kWordStart] with st + double(t_i) > current_end
__global__ __launch_bounds__(kBlock) void overlap_end_kernel(const float4* __restrict__ sec, uint32_t n, double st, double current_end,
                                                             unsigned* __restrict__ words) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || i <= words[kWordStart]) return;  // (no start: words[kWordStart] == n, nothing is behind it)
  if (__dadd_rn(st, static_cast<double>(sec[i].w)) > current_end) atomicMin(&words[kWordEnd], i);
}

// merged record j of m: the prior cloud's point j, or the secondary's point i_start + (j - n_primary) with
// t = float((double(t) + st) - current_end)
struct MergeArgs {
  const float4* primary;
  const float4* sec;
  uint32_t n_primary, i_start, m;
  double st, current_end;
};
__device__ __forceinline__ float4 merged_record(const MergeArgs& a, uint32_t j) {
  if (j < a.n_primary) return a.primary[j];
  float4 v = a.sec[a.i_start + (j - a.n_primary)];
  v.w = __double2float_rn(__dsub_rn(__dadd_rn(static_cast<double>(v.w), a.st), a.current_end));
  return v;
}

__global__ __launch_bounds__(kBlock) void merged_keys_kernel(MergeArgs a, float* __restrict__ keys) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j < a.m) keys[j] = merged_record(a, j).w;
}

// out[k] = merged record order[k] with its origin index, and the first and last t; nothing unless the sort succeeded
// (a refused sort leaves `order` unwritten)
__global__ __launch_bounds__(kBlock) void merged_gather_kernel(MergeArgs a, const int* __restrict__ order, const int* __restrict__ status,
                                                               float4* __restrict__ out, float* __restrict__ origin_index,
                                                               unsigned* __restrict__ words) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= a.m || *status != 0) return;
  const uint32_t j = static_cast<uint32_t>(order[k]);
  if (j >= a.m) return;  // (cannot happen: a permutation of 0 .. m - 1)
  const float4 v = merged_record(a, j);
  out[k] = v;
  origin_index[k] = j < a.n_primary ? 0.f : 1.f;
  if (k == 0u) words[kWordFront] = __float_as_uint(v.w);
  if (k + 1u == a.m) words[kWordBack] = __float_as_uint(v.w);
}

// common::ToSecondsStamp (common/time.cc:48-56) of universal-time ticks, as the adapter's Seconds()
double seconds_stamp(int64_t ticks) {
  constexpr int64_t kUtsEpochOffsetFromUnixEpochInSeconds = 719162ll * 24ll * 60ll * 60ll;
  const int64_t ns_since_unix_epoch = (ticks - kUtsEpochOffsetFromUnixEpochInSeconds * 10000000ll) * 100ll;
  return static_cast<double>(ns_since_unix_epoch) * 1e-9;
}

// a new object of n points in a block of the cloud pool, without intensities
int new_timed_cloud(dliom_ctx* ctx, int64_t n, bool with_origin_index, dliom_timed_cloud** out) {
  dliom_timed_cloud* cloud = new dliom_timed_cloud;
  cloud->ctx = ctx;
  cloud->device = ctx->device;
  cloud->has_origin_index = with_origin_index;
  cloud->n = n;
  if (n > 0) {
    const size_t nn = static_cast<size_t>(n);
    const int st = device_block_alloc(ctx->device, align256(16 * nn) + (with_origin_index ? 4 * nn : 0), &cloud->base, &cloud->base_bytes);
    if (st != DLIOM_OK) {
      delete cloud;
      return st;
    }
    cloud->d_xyzt = static_cast<float4*>(cloud->base);
    if (with_origin_index) cloud->d_origin_index = reinterpret_cast<float*>(static_cast<char*>(cloud->base) + align256(16 * nn));
  }
  *out = cloud;
  return DLIOM_OK;
}

// an input of stamp and merge: this context's, points and times only
bool plain_input(const dliom_timed_cloud* c, const dliom_ctx* ctx) {
  return c != nullptr && c->ctx == ctx && !c->has_intensities && !c->has_origin_index;
}

}  // namespace
}  // namespace dliom

using namespace dliom;

extern "C" {

int dliom_timed_cloud_stamp(dliom_ctx* ctx, const dliom_timed_cloud* in, double scan_period, dliom_timed_cloud** out) {
  if (ctx == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!plain_input(in, ctx) || !(scan_period > 0.) || !(scan_period < 1e30)) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  dliom_timed_cloud* cloud = nullptr;
  DLIOM_TRY(new_timed_cloud(ctx, in->n, false, &cloud));
  cloud->front_t = in->front_t;
  cloud->back_t = in->back_t;
  int st = DLIOM_OK;
  if (in->n == 1) {
    if (hipMemcpyAsync(cloud->d_xyzt, in->d_xyzt, 16, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) st = DLIOM_ERR_HIP;
  } else if (in->n >= 2) {
    const double duration = scan_period / static_cast<double>(in->n - 1);
    hipLaunchKernelGGL(stamp_kernel, dim3(blocks_of(in->n, kBlock)), dim3(kBlock), 0, ctx->stream, in->d_xyzt, static_cast<uint32_t>(in->n),
                       scan_period, duration, cloud->d_xyzt);
    if (hipGetLastError() != hipSuccess) st = DLIOM_ERR_HIP;
    cloud->front_t = static_cast<float>(-scan_period + 0 * duration);
    cloud->back_t = 0.f;
  }
  if (st != DLIOM_OK) {
    dliom_timed_cloud_destroy(cloud);
    return st;
  }
  *out = cloud;
  return DLIOM_OK;
}

int dliom_timed_clouds_merge(dliom_ctx* ctx, const dliom_timed_cloud* primary, const dliom_timed_cloud* primary_for_times,
                             int64_t primary_time, const dliom_timed_cloud* secondary, int64_t secondary_time, dliom_timed_cloud** out) {
  if (ctx == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!plain_input(primary, ctx) || !plain_input(secondary, ctx) || (primary_for_times != nullptr && !plain_input(primary_for_times, ctx)))
    return DLIOM_ERR_INVALID_ARGUMENT;
  const dliom_timed_cloud* timed = primary_for_times != nullptr ? primary_for_times : primary;
  if (timed->n != primary->n) return DLIOM_ERR_INVALID_ARGUMENT;
  const int64_t n_p = primary->n, n_s = secondary->n;
  if (n_s == 0) return DLIOM_ERR_INVALID_ARGUMENT;  // no i_start
  if (n_p > kMaxMerged) return DLIOM_ERR_CAPACITY;
  if (n_s >= (int64_t{1} << 27)) return DLIOM_ERR_INVALID_ARGUMENT;
  const double current_end = seconds_stamp(primary_time);
  const double current_start = n_p == 0 ? current_end : current_end + timed->front_t;
  const double st = seconds_stamp(secondary_time);
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  // words | the merged times (at most kMaxMerged of them are ever written)
  const size_t max_keys = static_cast<size_t>(std::min<int64_t>(n_p + n_s, kMaxMerged));
  DLIOM_TRY(ctx->outlier.reserve(256 + 4 * max_keys));
  unsigned* words = ctx->outlier.as<unsigned>();
  float* keys = reinterpret_cast<float*>(static_cast<char*>(ctx->outlier.p) + 256);
  const FillJob fill{words, 8, static_cast<unsigned>(n_s)};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  const unsigned sec_blocks = blocks_of(n_s, kBlock);
  hipLaunchKernelGGL(overlap_start_kernel, dim3(sec_blocks), dim3(kBlock), 0, ctx->stream, secondary->d_xyzt, static_cast<uint32_t>(n_s), st,
                     current_start, current_end, words);
  hipLaunchKernelGGL(overlap_end_kernel, dim3(sec_blocks), dim3(kBlock), 0, ctx->stream, secondary->d_xyzt, static_cast<uint32_t>(n_s), st,
                     current_end, words);
  DLIOM_HIP_TRY(hipGetLastError());
  unsigned* host = pinned_at<unsigned>(ctx, kPinReadback);
  const GatherJob bounds{words, 2};
  DLIOM_TRY(gather_and_wait(ctx, &bounds, 1, host));
  const int64_t i_start = host[kWordStart], i_end1 = host[kWordEnd];
  if (i_start >= n_s) return DLIOM_ERR_INVALID_ARGUMENT;  // CHECK(i_start != -1) (range_data_synchronizer.cc:84)
  if (i_end1 <= i_start || i_end1 > n_s) return DLIOM_ERR_HIP;  // (cannot happen)
  const int64_t m = n_p + (i_end1 - i_start);
  if (m > kMaxMerged) return DLIOM_ERR_CAPACITY;
  dliom_timed_cloud* cloud = nullptr;
  DLIOM_TRY(new_timed_cloud(ctx, m, true, &cloud));
  const MergeArgs a{primary->d_xyzt, secondary->d_xyzt, static_cast<uint32_t>(n_p), static_cast<uint32_t>(i_start), static_cast<uint32_t>(m),
                    st, current_end};
  const unsigned blocks = blocks_of(m, kBlock);
  int status = DLIOM_OK;
  hipLaunchKernelGGL(merged_keys_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, a, keys);
  if (hipGetLastError() != hipSuccess) status = DLIOM_ERR_HIP;
  const int *d_order = nullptr, *d_status = nullptr;
  if (status == DLIOM_OK) status = std_sort_order_enqueue(ctx, keys, static_cast<int>(m), &d_order, &d_status);
  if (status == DLIOM_OK) {
    hipLaunchKernelGGL(merged_gather_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, a, d_order, d_status, cloud->d_xyzt,
                       cloud->d_origin_index, words);
    if (hipGetLastError() != hipSuccess) status = DLIOM_ERR_HIP;
  }
  if (status == DLIOM_OK) {
    const GatherJob jobs[2] = {{d_status, 1}, {words + kWordFront, 2}};
    status = gather_and_wait(ctx, jobs, 2, host);
  }
  if (status == DLIOM_OK && host[0] != 0u) status = DLIOM_ERR_CAPACITY;  // the replay refuses this arrangement of equal times
  if (status != DLIOM_OK) {
    dliom_timed_cloud_destroy(cloud);
    return status;
  }
  std::memcpy(&cloud->front_t, &host[1], 4);
  std::memcpy(&cloud->back_t, &host[2], 4);
  *out = cloud;
  return DLIOM_OK;
}

}  // extern "C"
