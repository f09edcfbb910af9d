// XyzWriterPointsProcessor's per-point loop (io/xyz_writing_points_processor.cc:13-20) on the device: a batch's points as
// the text "x y z\n" a point, every coordinate float_text.h's text.  Records are 6 to 39 bytes
// long, so a record's place is known only after the lengths before it:
//   1. xyz_size_kernel   formats every point and leaves ONE total a workgroup (kTextPoints points);
//   2. hipcub's scan over the workgroups' totals (64-bit: 39 bytes * 2^31 points do not fit 32) -- the last entry is
//      the size of the text, read back through kPinReadback;
//   3. xyz_emit_kernel   formats again, places a workgroup's records in LDS by a scan of their lengths, and writes the
//      workgroup's range of the text as whole dwords.
// Byte offsets into the text are 64-bit everywhere; inside a workgroup they are below 256 * 39 + 3.
#include <hipcub/hipcub.hpp>

#include <cstring>

#include "device_common.h"
#include "float_text.h"
#include "pinned_layout.h"

namespace dliom {
namespace {

// Points a workgroup formats, one a lane.
constexpr int kTextPoints = 256;
constexpr int kMaxRecord = DLIOM_XYZ_MAX_RECORD;
static_assert(kMaxRecord == 3 * kFloatTextMax + 3, "three texts, two spaces, one newline");
// a workgroup's records, behind the 0 to 3 bytes that align its stage with the text's dwords
constexpr int kStageWords = (3 + kTextPoints * kMaxRecord + 3) / 4;

struct PointText {
  FloatText x, y, z;
  __device__ unsigned length() const { return static_cast<unsigned>(x.length + y.length + z.length + 3); }
};

__device__ __forceinline__ PointText point_text(const float* __restrict__ x, const float* __restrict__ y,
                                                const float* __restrict__ z, unsigned i) {
  PointText p;
  p.x = float_text_of_bits(__float_as_uint(x[i]));
  p.y = float_text_of_bits(__float_as_uint(y[i]));
  p.z = float_text_of_bits(__float_as_uint(z[i]));
  return p;
}

__global__ __launch_bounds__(kTextPoints) void xyz_size_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ z, unsigned n,
                                                               unsigned long long* __restrict__ totals) {
  using Reduce = hipcub::BlockReduce<unsigned, kTextPoints>;
  __shared__ typename Reduce::TempStorage temp;
  const unsigned i = blockIdx.x * kTextPoints + threadIdx.x;
  const unsigned length = i < n ? point_text(x, y, z, i).length() : 0u;
  const unsigned total = Reduce(temp).Sum(length);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

__device__ __forceinline__ unsigned put_text(unsigned char* at, const FloatText& t, unsigned end_char) {
  for (int k = 0; k < t.length; ++k) at[k] = static_cast<unsigned char>(ft_char(t, k));
  at[t.length] = static_cast<unsigned char>(end_char);
  return static_cast<unsigned>(t.length) + 1u;
}

// inclusive[g]: the bytes of the workgroups 0 to g.  Workgroup g owns the bytes [first, first + total) of the text, first =
// inclusive[g - 1]; its stage holds them from byte `pad` = first % 4 on, so that a dword of the stage IS a dword of the
// text (`out` is 256-byte aligned).  Dwords that lie wholly inside the range go out as dwords, one a lane, coalesced.  The
// first and the last dword may be shared with the neighbouring workgroups: of those only the bytes inside the range are
// stored, as bytes -- a dword store there, or a read-modify-write, would race with the neighbour's.
__global__ __launch_bounds__(kTextPoints) void xyz_emit_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ z, unsigned n,
                                                               const unsigned long long* __restrict__ inclusive,
                                                               unsigned char* __restrict__ out) {
  using Scan = hipcub::BlockScan<unsigned, kTextPoints>;
  __shared__ typename Scan::TempStorage temp;
  __shared__ unsigned stage[kStageWords];
  unsigned char* bytes = reinterpret_cast<unsigned char*>(stage);
  const unsigned i = blockIdx.x * kTextPoints + threadIdx.x;
  const unsigned long long first = blockIdx.x > 0 ? inclusive[blockIdx.x - 1] : 0ull;
  // (the sizing pass's total: never above kTextPoints * kMaxRecord, which is what the stage holds)
  const unsigned total = static_cast<unsigned>(min(inclusive[blockIdx.x] - first, static_cast<unsigned long long>(kTextPoints * kMaxRecord)));
  const unsigned pad = static_cast<unsigned>(first & 3ull);
  PointText p{};
  unsigned length = 0;
  if (i < n) {
    p = point_text(x, y, z, i);
    length = p.length();
  }
  unsigned before;
  Scan(temp).ExclusiveSum(length, before);
  if (i < n && before + length <= total) {  // (always: the sizing pass made `total` from the same lengths)
    unsigned char* at = bytes + pad + before;
    at += put_text(at, p.x, ' ');
    at += put_text(at, p.y, ' ');
    put_text(at, p.z, '\n');
  }
  __syncthreads();
  const unsigned end = pad + total;  // of the range, in stage bytes
  unsigned* out_words = reinterpret_cast<unsigned*>(out + (first - pad));
  unsigned char* out_bytes = out + (first - pad);
  for (unsigned w = threadIdx.x; 4u * w < end; w += kTextPoints) {
    if (4u * w >= pad && 4u * w + 4u <= end) {
      out_words[w] = stage[w];
    } else {
      for (unsigned b = 4u * w; b < 4u * w + 4u; ++b)
        if (b >= pad && b < end) out_bytes[b] = bytes[b];
    }
  }
}

// sizes of the scratch in ctx->outlier: totals | inclusive | hipcub's | the text
struct TextScratch {
  unsigned long long *totals, *inclusive;
  void* tmp;
  size_t tmp_bytes, head_bytes;
};

int carve_text(dliom_ctx* ctx, unsigned groups, size_t text_bytes, TextScratch* s) {
  size_t tmp = 0;
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tmp, static_cast<const unsigned long long*>(nullptr),
                                                 static_cast<unsigned long long*>(nullptr), static_cast<int>(groups), ctx->stream));
  const size_t per = align256(8 * static_cast<size_t>(groups));
  s->tmp_bytes = tmp;
  s->head_bytes = 2 * per + align256(tmp);
  DLIOM_TRY(ctx->outlier.reserve(s->head_bytes + align256(text_bytes)));
  char* b = static_cast<char*>(ctx->outlier.p);
  s->totals = reinterpret_cast<unsigned long long*>(b);
  s->inclusive = reinterpret_cast<unsigned long long*>(b + per);
  s->tmp = b + 2 * per;
  return DLIOM_OK;
}

int enqueue_sizes(dliom_ctx* ctx, const dliom_cloud* cloud, unsigned groups, const TextScratch& s) {
  hipLaunchKernelGGL(xyz_size_kernel, dim3(groups), dim3(kTextPoints), 0, ctx->stream, cloud->d_x, cloud->d_y, cloud->d_z,
                     static_cast<unsigned>(cloud->n), s.totals);
  DLIOM_HIP_TRY(hipGetLastError());
  size_t tmp = s.tmp_bytes;
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(s.tmp, tmp, s.totals, s.inclusive, static_cast<int>(groups), ctx->stream));
  return DLIOM_OK;
}

int pack_xyz(const dliom_cloud* cloud, uint8_t* bytes, int64_t capacity, int64_t* num_bytes) {
  if (cloud == nullptr || num_bytes == nullptr || capacity < 0 || cloud->n > INT32_MAX) return DLIOM_ERR_INVALID_ARGUMENT;
  *num_bytes = 0;
  const int64_t n = cloud->n;
  if (n == 0) return DLIOM_OK;  // the writer passes an empty batch on before it looks at it
  dliom_ctx* ctx = cloud->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const unsigned groups = dliom::blocks_of(n, kTextPoints);
  TextScratch s;
  // Room for the text the buffer can take, and never more than the longest text: mostly the emit pass then finds its
  // room already there.  (What the text really needs is known only after the read-back.)
  const int64_t longest = n * kMaxRecord;
  DLIOM_TRY(carve_text(ctx, groups, bytes != nullptr ? static_cast<size_t>(capacity < longest ? capacity : longest) : 0, &s));
  DLIOM_TRY(enqueue_sizes(ctx, cloud, groups, s));
  unsigned* host = pinned_at<unsigned>(ctx, kPinReadback);
  const GatherJob job{s.inclusive + (groups - 1), 2};
  DLIOM_TRY(gather_and_wait(ctx, &job, 1, host));
  unsigned long long total;
  std::memcpy(&total, host, 8);
  *num_bytes = static_cast<int64_t>(total);
  if (bytes == nullptr) return DLIOM_OK;
  if (capacity < *num_bytes) return DLIOM_ERR_CAPACITY;
  unsigned char* text = static_cast<unsigned char*>(ctx->outlier.p) + s.head_bytes;
  hipLaunchKernelGGL(xyz_emit_kernel, dim3(groups), dim3(kTextPoints), 0, ctx->stream, cloud->d_x, cloud->d_y, cloud->d_z,
                     static_cast<unsigned>(n), s.inclusive, text);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipMemcpyAsync(bytes, text, static_cast<size_t>(total), hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  return DLIOM_OK;
}

}  // namespace
}  // namespace dliom

extern "C" {

int dliom_float_text(float value, char buffer[16], int32_t* length) {
  if (buffer == nullptr || length == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  uint32_t bits;
  std::memcpy(&bits, &value, 4);
  const dliom::FloatText t = dliom::float_text_of_bits(bits);
  for (int i = 0; i < t.length; ++i) buffer[i] = static_cast<char>(dliom::ft_char(t, i));
  *length = t.length;
  return DLIOM_OK;
}

int dliom_points_batch_pack_xyz(const dliom_points_batch* batch, uint8_t* bytes, int64_t capacity, int64_t* num_bytes) {
  if (batch == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  return dliom::pack_xyz(batch->cloud, bytes, capacity, num_bytes);
}

int dliom_cloud_pack_xyz(const dliom_cloud* cloud, uint8_t* bytes, int64_t capacity, int64_t* num_bytes) {
  return dliom::pack_xyz(cloud, bytes, capacity, num_bytes);
}

}  // extern "C"
