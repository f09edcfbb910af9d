// sensor::CompressedPointCloud and mapping::proto::TrajectoryNodeData on the device (dliom.h "compressed point clouds";
// DESIGN.md section 3.19).  One code path, the batched one: K clouds of a context are keyed, sorted, emitted and varint
// packed together; a single cloud is a batch of one.
//   keys      a point: the bound check, q = lround(p / 0.001f) an axis, the 42-bit block key under its cloud's index, the
//             30-bit word of the offsets
//   sort      stable radix sort of (key, point index) over the key bits in use: points of a block keep their input order
//   emission  segment heads -> scan -> the int32 streams of all clouds in one buffer, with word offsets a cloud
//   packing   bytes a point (its word, and its block's header in front of the first) -> scan -> the varints of every
//             cloud's field 3, with byte offsets a cloud
// The host frames messages around the payloads and never loops over words.  Decompression: the host walks the words (or
// the varints, sequential by nature), the device writes a point a thread.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_common.h"
#include "proto_wire.h"

namespace dliom {
namespace {

constexpr int kBlock = 256;
constexpr float kPrecision = 0.001f;
constexpr int kBlockKeyBits = 42;
constexpr int64_t kMaxBatchPoints = int64_t{1} << 26;  // 5 words a point at most: stream indices stay below 2^31
constexpr int kMaxBatchClouds = 1 << 20;
constexpr unsigned kNoCloud = 0xFFFFFFFFu;

// meta words of a batch, read back in one copy: [first refused cloud | blocks | word_off[k + 1] | byte_off[k + 1]]
constexpr int kMetaRefused = 0, kMetaBlocks = 1, kMetaOffsets = 2;

struct CloudTable {
  const unsigned* pt_off;  // k + 1: first point of cloud c in the batch's numbering
  const float* const* x;   // k each
  const float* const* y;
  const float* const* z;
};

// the cloud of point i: the largest c with pt_off[c] <= i (an empty cloud is never that)
__device__ __forceinline__ unsigned cloud_of(const unsigned* __restrict__ pt_off, unsigned k, unsigned i) {
  unsigned lo = 0, hi = k;
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (pt_off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// HybridGridBase's iterator order of the block (bx, by, bz), each in [-8192, 8191]: z-major at each of the three levels
__device__ __forceinline__ uint64_t block_key(int bx, int by, int bz) {
  const unsigned X = static_cast<unsigned>(bx + 8192), Y = static_cast<unsigned>(by + 8192), Z = static_cast<unsigned>(bz + 8192);
  const uint64_t meta = (Z >> 6) << 16 | (Y >> 6) << 8 | (X >> 6);
  const uint64_t leaf = ((Z >> 3) & 7u) << 6 | ((Y >> 3) & 7u) << 3 | ((X >> 3) & 7u);
  const uint64_t cell = (Z & 7u) << 6 | (Y & 7u) << 3 | (X & 7u);
  return meta << 18 | leaf << 9 | cell;
}
__device__ __forceinline__ int key_axis(uint64_t key, int axis) {  // axis 0 x, 1 y, 2 z
  const unsigned meta = static_cast<unsigned>(key >> (18 + 8 * axis)) & 0xFFu;
  const unsigned leaf = static_cast<unsigned>(key >> (9 + 3 * axis)) & 7u;
  const unsigned cell = static_cast<unsigned>(key >> (3 * axis)) & 7u;
  return static_cast<int>(meta << 6 | leaf << 3 | cell) - 8192;
}

__device__ __forceinline__ bool in_bound(float p) { return fabsf(p) / kPrecision < 8388608.f; }  // false for NaN, +-inf

__global__ __launch_bounds__(kBlock) void compress_keys_kernel(CloudTable t, unsigned k, unsigned n, uint64_t* __restrict__ keys,
                                                               unsigned* __restrict__ index, unsigned* __restrict__ words,
                                                               unsigned* __restrict__ refused) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned c = cloud_of(t.pt_off, k, i);
  const unsigned j = i - t.pt_off[c];
  const float x = t.x[c][j], y = t.y[c][j], z = t.z[c][j];
  const bool ok = in_bound(x) && in_bound(y) && in_bound(z);
  if (!ok) atomicMin(refused, c);
  // a refused point takes the origin's key: the call is refused, but everything behind this kernel stays in bounds
  const int qx = ok ? cell_of(x, kPrecision) : 0, qy = ok ? cell_of(y, kPrecision) : 0, qz = ok ? cell_of(z, kPrecision) : 0;
  keys[i] = static_cast<uint64_t>(c) << kBlockKeyBits | block_key(qx >> 10, qy >> 10, qz >> 10);
  index[i] = i;
  words[i] = (static_cast<unsigned>(qz & 1023) << 10 | static_cast<unsigned>(qy & 1023)) << 10 | static_cast<unsigned>(qx & 1023);
}

__global__ __launch_bounds__(kBlock) void compress_heads_kernel(const uint64_t* __restrict__ keys, unsigned n, unsigned* __restrict__ head) {
  const unsigned s = blockIdx.x * kBlock + threadIdx.x;
  if (s < n) head[s] = s == 0u || keys[s] != keys[s - 1] ? 1u : 0u;
}

// head_pos[b] = the sorted position of block b's first point, head_pos[blocks] = n
__global__ __launch_bounds__(kBlock) void compress_block_starts_kernel(const unsigned* __restrict__ head, const unsigned* __restrict__ inclusive,
                                                                       unsigned n, unsigned* __restrict__ head_pos) {
  const unsigned s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n) return;
  if (head[s] != 0u) head_pos[inclusive[s] - 1u] = s;
  if (s == n - 1u) head_pos[inclusive[s]] = n;
}

__device__ __forceinline__ unsigned varint_bytes(int v) {  // an int32 on the wire: sign-extended to 64 bits
  const unsigned u = static_cast<unsigned>(v);
  return v < 0 ? 10u : 1u + (u >= 1u << 7) + (u >= 1u << 14) + (u >= 1u << 21) + (u >= 1u << 28);
}

// Sorted point s of block b: its word at stream[s + 4 (b + 1)], the block's header (count, x, y, z) in front of the
// first.  point_bytes[s]: the varint bytes of what this thread wrote.  Threads [n, n + k]: the clouds' word offsets.
__global__ __launch_bounds__(kBlock) void compress_emit_kernel(const uint64_t* __restrict__ keys, const unsigned* __restrict__ index,
                                                               const unsigned* __restrict__ words, const unsigned* __restrict__ head,
                                                               const unsigned* __restrict__ inclusive, const unsigned* __restrict__ head_pos,
                                                               const unsigned* __restrict__ pt_off, unsigned k, unsigned n,
                                                               int32_t* __restrict__ stream, unsigned* __restrict__ point_bytes,
                                                               unsigned* __restrict__ meta) {
  const unsigned s = blockIdx.x * kBlock + threadIdx.x;
  if (s < n) {
    const unsigned b = inclusive[s] - 1u;
    const int word = static_cast<int>(words[index[s]]);
    unsigned bytes = varint_bytes(word);
    if (head[s] != 0u) {
      const uint64_t key = keys[s];
      int32_t* h = stream + (s + 4u * b);
      h[0] = static_cast<int>(head_pos[b + 1u] - s);
      h[1] = key_axis(key, 0);
      h[2] = key_axis(key, 1);
      h[3] = key_axis(key, 2);
      bytes += varint_bytes(h[0]) + varint_bytes(h[1]) + varint_bytes(h[2]) + varint_bytes(h[3]);
    }
    stream[s + 4u * (b + 1u)] = word;
    point_bytes[s] = bytes;
  } else if (s - n <= k) {
    const unsigned c = s - n, p = pt_off[c], blocks = inclusive[n - 1u];
    meta[kMetaOffsets + c] = p + 4u * (p < n ? inclusive[p] - 1u : blocks);  // a cloud's first point heads a block
    if (c == k) meta[kMetaBlocks] = blocks;
  }
}

__global__ __launch_bounds__(kBlock) void compress_byte_offsets_kernel(const unsigned* __restrict__ point_bytes,
                                                                       const unsigned* __restrict__ bytes_inclusive,
                                                                       const unsigned* __restrict__ pt_off, unsigned k, unsigned n,
                                                                       unsigned* __restrict__ byte_off) {
  const unsigned c = blockIdx.x * kBlock + threadIdx.x;
  if (c > k) return;
  const unsigned p = pt_off[c];
  byte_off[c] = p < n ? bytes_inclusive[p] - point_bytes[p] : bytes_inclusive[n - 1u];
}

__device__ __forceinline__ uint8_t* put_varint_device(uint8_t* out, int v) {
  uint64_t u = static_cast<uint64_t>(static_cast<int64_t>(v));
  while (u >= 0x80u) {
    *out++ = static_cast<uint8_t>(u) | 0x80u;
    u >>= 7;
  }
  *out++ = static_cast<uint8_t>(u);
  return out;
}

__global__ __launch_bounds__(kBlock) void compress_pack_kernel(const int32_t* __restrict__ stream, const unsigned* __restrict__ head,
                                                               const unsigned* __restrict__ inclusive, const unsigned* __restrict__ point_bytes,
                                                               const unsigned* __restrict__ bytes_inclusive, unsigned n,
                                                               uint8_t* __restrict__ out) {
  const unsigned s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n) return;
  const unsigned b = inclusive[s] - 1u;
  uint8_t* o = out + (bytes_inclusive[s] - point_bytes[s]);
  if (head[s] != 0u) {
    const int32_t* h = stream + (s + 4u * b);
    for (int f = 0; f < 4; ++f) o = put_varint_device(o, h[f]);
  }
  put_varint_device(o, stream[s + 4u * (b + 1u)]);
}

// One thread a point: its block by bisection of the blocks' first points, ReadNextPoint's arithmetic
__global__ __launch_bounds__(kBlock) void decompress_kernel(const int32_t* __restrict__ stream, const unsigned* __restrict__ block_first,
                                                            unsigned blocks, unsigned n, float* __restrict__ x, float* __restrict__ y,
                                                            float* __restrict__ z, unsigned* __restrict__ maxima) {
  const unsigned p = blockIdx.x * kBlock + threadIdx.x;
  unsigned sq = 0u, ax = 0u, ay = 0u, az = 0u;
  if (p < n) {
    const unsigned b = cloud_of(block_first, blocks, p);
    const int32_t* h = stream + (block_first[b] + 4u * b);
    const unsigned w = static_cast<unsigned>(stream[p + 4u * (b + 1u)]);
    // (block << 10) + offset in 32-bit two's complement, whatever the stream's block coordinates are
    const int qx = static_cast<int>((static_cast<unsigned>(h[1]) << 10) + (w & 1023u));
    const int qy = static_cast<int>((static_cast<unsigned>(h[2]) << 10) + ((w >> 10) & 1023u));
    const int qz = static_cast<int>((static_cast<unsigned>(h[3]) << 10) + (w >> 20));
    const float fx = static_cast<float>(qx) * kPrecision, fy = static_cast<float>(qy) * kPrecision, fz = static_cast<float>(qz) * kPrecision;
    x[p] = fx;
    y[p] = fy;
    z[p] = fz;
    sq = norm_word(fx, fy, fz);
    ax = __float_as_uint(fabsf(fx));
    ay = __float_as_uint(fabsf(fy));
    az = __float_as_uint(fabsf(fz));
  }
  note_kept(sq, maxima);
  note_kept(ax, maxima + 1);
  note_kept(ay, maxima + 2);
  note_kept(az, maxima + 3);
}

bool launched() { return hipGetLastError() == hipSuccess; }

struct Batch {
  int64_t n = 0;
  int k = 0;
  std::vector<unsigned> meta;  // as read back
  const int32_t* d_stream = nullptr;
  // what the packing needs
  const unsigned *d_head = nullptr, *d_inclusive = nullptr, *d_point_bytes = nullptr, *d_bytes_inclusive = nullptr;
  int64_t words() const { return meta[kMetaOffsets + k]; }
  int64_t bytes() const { return meta[kMetaOffsets + (k + 1) + k]; }
  int64_t word_off(int c) const { return meta[kMetaOffsets + c]; }
  int64_t byte_off(int c) const { return meta[kMetaOffsets + (k + 1) + c]; }
};

int check_clouds(const dliom_ctx* ctx, const dliom_cloud* const* clouds, int k, int64_t* total) {
  if (ctx == nullptr || k < 0 || k > kMaxBatchClouds || (k > 0 && clouds == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  int64_t n = 0;
  for (int c = 0; c < k; ++c) {
    if (clouds[c] == nullptr) continue;  // NULL: the empty cloud
    if (clouds[c]->device != ctx->device || clouds[c]->n < 0) return DLIOM_ERR_INVALID_ARGUMENT;
    n += clouds[c]->n;
    if (n > kMaxBatchPoints) return DLIOM_ERR_TOO_LARGE;
  }
  *total = n;
  return DLIOM_OK;
}

// Keys, sort, emission and (with_bytes) the byte counts of the batch on ctx->stream, then the call's one read-back of
// sizes: b->meta.  The streams stay in ctx->compress until the context's next batch.
int run_batch(dliom_ctx* ctx, const dliom_cloud* const* clouds, int k, bool with_bytes, Batch* b) {
  DLIOM_TRY(check_clouds(ctx, clouds, k, &b->n));
  b->k = k;
  const size_t n = static_cast<size_t>(b->n), k1 = static_cast<size_t>(k) + 1;
  b->meta.assign(kMetaOffsets + 2 * k1, 0u);
  b->meta[kMetaRefused] = kNoCloud;
  if (n == 0) return DLIOM_OK;  // every stream is empty: all offsets are zero
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));

  std::vector<unsigned> pt_off(k1);
  std::vector<const float*> ptrs(3 * static_cast<size_t>(k), nullptr);
  for (int c = 0; c < k; ++c) {
    pt_off[c + 1] = pt_off[c] + (clouds[c] != nullptr ? static_cast<unsigned>(clouds[c]->n) : 0u);
    if (clouds[c] == nullptr) continue;
    ptrs[c] = clouds[c]->d_x;
    ptrs[k + c] = clouds[c]->d_y;
    ptrs[2 * static_cast<size_t>(k) + c] = clouds[c]->d_z;
  }

  int end_bit = kBlockKeyBits;
  while ((int64_t{1} << (end_bit - kBlockKeyBits)) < k) ++end_bit;  // the cloud index's bits in use
  size_t sort_tmp = 0, scan_tmp = 0;
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                                   static_cast<const unsigned*>(nullptr), static_cast<unsigned*>(nullptr),
                                                   static_cast<int>(n), 0, end_bit, ctx->stream));
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_tmp, static_cast<const unsigned*>(nullptr), static_cast<unsigned*>(nullptr),
                                                 static_cast<int>(n), ctx->stream));
  DLIOM_TRY(ctx->sort_tmp.reserve(std::max(sort_tmp, scan_tmp)));

  const size_t per = align256(4 * (n + 1));
  const size_t at_keys_in = 0, at_keys_out = at_keys_in + 2 * per, at_index_in = at_keys_out + 2 * per, at_index_out = at_index_in + per,
               at_words = at_index_out + per, at_head = at_words + per, at_inclusive = at_head + per, at_head_pos = at_inclusive + per,
               at_point_bytes = at_head_pos + per, at_bytes_inclusive = at_point_bytes + per, at_stream = at_bytes_inclusive + per,
               at_pt_off = at_stream + align256(20 * n), at_ptrs = at_pt_off + align256(4 * k1),
               at_meta = at_ptrs + align256(8 * ptrs.size()), total = at_meta + align256(4 * b->meta.size());
  DLIOM_TRY(ctx->compress.reserve(total));
  char* base = static_cast<char*>(ctx->compress.p);
  auto at = [&](size_t off) { return static_cast<void*>(base + off); };
  uint64_t *keys_in = static_cast<uint64_t*>(at(at_keys_in)), *keys_out = static_cast<uint64_t*>(at(at_keys_out));
  unsigned *index_in = static_cast<unsigned*>(at(at_index_in)), *index_out = static_cast<unsigned*>(at(at_index_out)),
           *words = static_cast<unsigned*>(at(at_words)), *head = static_cast<unsigned*>(at(at_head)),
           *inclusive = static_cast<unsigned*>(at(at_inclusive)), *head_pos = static_cast<unsigned*>(at(at_head_pos)),
           *point_bytes = static_cast<unsigned*>(at(at_point_bytes)), *bytes_inclusive = static_cast<unsigned*>(at(at_bytes_inclusive)),
           *d_pt_off = static_cast<unsigned*>(at(at_pt_off)), *d_meta = static_cast<unsigned*>(at(at_meta));
  int32_t* stream = static_cast<int32_t*>(at(at_stream));
  const float* const* d_ptrs = static_cast<const float* const*>(at(at_ptrs));

  DLIOM_HIP_TRY(hipMemcpyAsync(d_pt_off, pt_off.data(), 4 * k1, hipMemcpyHostToDevice, ctx->stream));
  DLIOM_HIP_TRY(hipMemcpyAsync(at(at_ptrs), ptrs.data(), 8 * ptrs.size(), hipMemcpyHostToDevice, ctx->stream));
  const FillJob fill{d_meta, 4, kNoCloud};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));

  const unsigned un = static_cast<unsigned>(n), uk = static_cast<unsigned>(k);
  const dim3 grid(blocks_of(b->n, kBlock)), block(kBlock);
  const CloudTable table{d_pt_off, d_ptrs, d_ptrs + k, d_ptrs + 2 * static_cast<size_t>(k)};
  hipLaunchKernelGGL(compress_keys_kernel, grid, block, 0, ctx->stream, table, uk, un, keys_in, index_in, words, d_meta + kMetaRefused);
  if (!launched()) return DLIOM_ERR_HIP;
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(ctx->sort_tmp.p, sort_tmp, keys_in, keys_out, index_in, index_out, static_cast<int>(n), 0,
                                                   end_bit, ctx->stream));
  hipLaunchKernelGGL(compress_heads_kernel, grid, block, 0, ctx->stream, keys_out, un, head);
  if (!launched()) return DLIOM_ERR_HIP;
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(ctx->sort_tmp.p, scan_tmp, head, inclusive, static_cast<int>(n), ctx->stream));
  hipLaunchKernelGGL(compress_block_starts_kernel, grid, block, 0, ctx->stream, head, inclusive, un, head_pos);
  if (!launched()) return DLIOM_ERR_HIP;
  hipLaunchKernelGGL(compress_emit_kernel, dim3(blocks_of(b->n + k + 1, kBlock)), block, 0, ctx->stream, keys_out, index_out, words, head,
                     inclusive, head_pos, d_pt_off, uk, un, stream, point_bytes, d_meta);
  if (!launched()) return DLIOM_ERR_HIP;
  if (with_bytes) {
    DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(ctx->sort_tmp.p, scan_tmp, point_bytes, bytes_inclusive, static_cast<int>(n), ctx->stream));
    hipLaunchKernelGGL(compress_byte_offsets_kernel, dim3(blocks_of(k + 1, kBlock)), block, 0, ctx->stream, point_bytes, bytes_inclusive,
                       d_pt_off, uk, un, d_meta + kMetaOffsets + k1);
    if (!launched()) return DLIOM_ERR_HIP;
  }
  const size_t meta_words = kMetaOffsets + (with_bytes ? 2 : 1) * k1;
  DLIOM_HIP_TRY(hipMemcpyAsync(b->meta.data(), d_meta, 4 * meta_words, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  b->d_stream = stream;
  b->d_head = head;
  b->d_inclusive = inclusive;
  b->d_point_bytes = point_bytes;
  b->d_bytes_inclusive = bytes_inclusive;
  return DLIOM_OK;
}

// The varint payloads of every cloud's field 3, back to back (b.bytes() of them), brought down into the context's
// page-locked batch block: *host points there until the context's next batched call.
int pack_batch(dliom_ctx* ctx, const Batch& b, const uint8_t** host) {
  *host = nullptr;
  if (b.bytes() == 0) return DLIOM_OK;
  DLIOM_TRY(ctx->compress_out.reserve(static_cast<size_t>(b.bytes())));
  DLIOM_TRY(ctx->reserve_batch_pinned(static_cast<size_t>(b.bytes())));
  uint8_t* out = ctx->compress_out.as<uint8_t>();
  hipLaunchKernelGGL(compress_pack_kernel, dim3(blocks_of(b.n, kBlock)), dim3(kBlock), 0, ctx->stream, b.d_stream, b.d_head, b.d_inclusive,
                     b.d_point_bytes, b.d_bytes_inclusive, static_cast<unsigned>(b.n), out);
  if (!launched()) return DLIOM_ERR_HIP;
  DLIOM_HIP_TRY(hipMemcpyAsync(ctx->batch_pinned, out, static_cast<size_t>(b.bytes()), hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  *host = static_cast<const uint8_t*>(ctx->batch_pinned);
  return DLIOM_OK;
}

int64_t cloud_points(const dliom_cloud* c) { return c != nullptr ? c->n : 0; }

uint8_t* put_varint_at(uint8_t* out, uint64_t v) {
  while (v >= 0x80) {
    *out++ = static_cast<uint8_t>(v) | 0x80;
    v >>= 7;
  }
  *out++ = static_cast<uint8_t>(v);
  return out;
}
// sensor::proto::CompressedPointCloud around a field-3 payload that is already varint bytes: its size, and the message
// written at `out` (the one pass over the payload that the host makes)
int64_t compressed_cloud_size(int64_t num_points, int64_t payload_bytes) {
  int64_t s = num_points != 0 ? 1 + wire::varint_size(static_cast<uint64_t>(num_points)) : 0;
  if (payload_bytes > 0) s += 1 + wire::varint_size(static_cast<uint64_t>(payload_bytes)) + payload_bytes;
  return s;
}
uint8_t* put_compressed_cloud(uint8_t* out, int64_t num_points, const uint8_t* payload, int64_t payload_bytes) {
  if (num_points != 0) {
    *out++ = 1u << 3 | 0;
    out = put_varint_at(out, static_cast<uint64_t>(num_points));  // (int32: sign-extended; never negative here)
  }
  if (payload_bytes > 0) {
    *out++ = 3u << 3 | 2;
    out = put_varint_at(out, static_cast<uint64_t>(payload_bytes));
    std::memcpy(out, payload, static_cast<size_t>(payload_bytes));
    out += payload_bytes;
  }
  return out;
}

// Compress's stream, checked as dliom.h states it: blocks' first points into block_first (blocks + 1 entries)
int walk_stream(int32_t num_points, const int32_t* point_data, int64_t n, std::vector<unsigned>* block_first) {
  if (num_points < 0 || n < 0 || (n > 0 && point_data == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  block_first->clear();
  int64_t i = 0, points = 0;
  while (i < n) {
    if (n - i < 4) return DLIOM_ERR_INVALID_ARGUMENT;  // ends inside a header
    const int64_t count = point_data[i];
    if (count <= 0 || count > n - i - 4) return DLIOM_ERR_INVALID_ARGUMENT;  // ... inside a block
    for (int64_t j = i + 4; j < i + 4 + count; ++j)
      if ((static_cast<uint32_t>(point_data[j]) >> 30) != 0u) return DLIOM_ERR_INVALID_ARGUMENT;
    block_first->push_back(static_cast<unsigned>(points));
    points += count;
    if (points > num_points) return DLIOM_ERR_INVALID_ARGUMENT;  // trailing words, or counts beyond num_points
    i += 4 + count;
  }
  if (points != num_points) return DLIOM_ERR_INVALID_ARGUMENT;
  block_first->push_back(static_cast<unsigned>(points));
  return DLIOM_OK;
}

// sensor::proto::CompressedPointCloud: field 1 num_points, field 3 point_data (packed or not), anything else skipped
int parse_compressed_cloud(const uint8_t* p, const uint8_t* end, int32_t* num_points, std::vector<int32_t>* point_data) {
  *num_points = 0;
  point_data->clear();
  while (p < end) {
    uint64_t tag, v;
    if (!wire::get_varint(p, end, &tag)) return DLIOM_ERR_INVALID_ARGUMENT;
    const unsigned wire_type = static_cast<unsigned>(tag & 7);
    const uint64_t field = tag >> 3;
    if (field == 1 && wire_type == 0) {
      if (!wire::get_varint(p, end, &v)) return DLIOM_ERR_INVALID_ARGUMENT;
      *num_points = static_cast<int32_t>(v);
    } else if (field == 3 && wire_type == 0) {
      if (!wire::get_varint(p, end, &v)) return DLIOM_ERR_INVALID_ARGUMENT;
      point_data->push_back(static_cast<int32_t>(v));
    } else if (field == 3 && wire_type == 2) {
      if (!wire::get_varint(p, end, &v) || static_cast<uint64_t>(end - p) < v) return DLIOM_ERR_INVALID_ARGUMENT;
      const uint8_t* qe = p + v;
      while (p < qe) {
        if (!wire::get_varint(p, qe, &v)) return DLIOM_ERR_INVALID_ARGUMENT;
        point_data->push_back(static_cast<int32_t>(v));
      }
    } else if (!wire::skip_field(p, end, wire_type)) {
      return DLIOM_ERR_INVALID_ARGUMENT;
    }
  }
  return DLIOM_OK;
}

int check_buffer(const uint8_t* bytes, int64_t size) { return size < 0 || (size > 0 && bytes == nullptr) ? DLIOM_ERR_INVALID_ARGUMENT : DLIOM_OK; }

int deliver(const std::vector<uint8_t>& msg, uint8_t* buffer, int64_t capacity, int64_t* size) {
  *size = static_cast<int64_t>(msg.size());
  if (buffer == nullptr) return DLIOM_OK;  // size query
  if (capacity < *size) return DLIOM_ERR_CAPACITY;
  if (!msg.empty()) std::memcpy(buffer, msg.data(), msg.size());
  return DLIOM_OK;
}

}  // namespace
}  // namespace dliom

using namespace dliom;

extern "C" int dliom_clouds_compress(dliom_ctx* ctx, const dliom_cloud* const* clouds, int k, int32_t* point_data, int64_t capacity,
                                     int64_t* word_offsets, int* first_refused) {
  if (word_offsets == nullptr || first_refused == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  *first_refused = -1;
  Batch b;
  DLIOM_TRY(run_batch(ctx, clouds, k, false, &b));
  if (b.meta[kMetaRefused] != kNoCloud) {
    *first_refused = static_cast<int>(b.meta[kMetaRefused]);
    return DLIOM_ERR_GRID_EXTENT;
  }
  for (int c = 0; c <= k; ++c) word_offsets[c] = b.word_off(c);
  if (point_data == nullptr) return DLIOM_OK;  // size query
  if (capacity < b.words()) return DLIOM_ERR_CAPACITY;
  if (b.words() > 0) {
    DLIOM_HIP_TRY(hipMemcpyAsync(point_data, b.d_stream, 4 * static_cast<size_t>(b.words()), hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    ++ctx->host_syncs;
  }
  return DLIOM_OK;
}

extern "C" int dliom_cloud_compress(dliom_ctx* ctx, const dliom_cloud* cloud, int32_t* point_data, int64_t capacity, int64_t* size) {
  if (cloud == nullptr || size == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  int64_t offsets[2] = {0, 0};
  int refused = -1;
  const int st = dliom_clouds_compress(ctx, &cloud, 1, point_data, capacity, offsets, &refused);
  if (st == DLIOM_OK || st == DLIOM_ERR_CAPACITY) *size = offsets[1];
  return st;
}

extern "C" int dliom_clouds_compress_to_proto(dliom_ctx* ctx, const dliom_cloud* const* clouds, int k, uint8_t* bytes, int64_t capacity,
                                              int64_t* byte_offsets, int* first_refused) {
  if (byte_offsets == nullptr || first_refused == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  *first_refused = -1;
  Batch b;
  DLIOM_TRY(run_batch(ctx, clouds, k, true, &b));
  if (b.meta[kMetaRefused] != kNoCloud) {
    *first_refused = static_cast<int>(b.meta[kMetaRefused]);
    return DLIOM_ERR_GRID_EXTENT;
  }
  int64_t at = 0;
  for (int c = 0; c < k; ++c) {
    byte_offsets[c] = at;
    at += compressed_cloud_size(cloud_points(clouds[c]), b.byte_off(c + 1) - b.byte_off(c));
  }
  byte_offsets[k] = at;
  if (bytes == nullptr) return DLIOM_OK;  // size query
  if (capacity < at) return DLIOM_ERR_CAPACITY;
  const uint8_t* payload = nullptr;
  DLIOM_TRY(pack_batch(ctx, b, &payload));
  uint8_t* out = bytes;
  for (int c = 0; c < k; ++c) out = put_compressed_cloud(out, cloud_points(clouds[c]), payload + b.byte_off(c), b.byte_off(c + 1) - b.byte_off(c));
  return DLIOM_OK;
}

extern "C" int dliom_compressed_point_cloud_to_proto(int32_t num_points, const int32_t* point_data, int64_t n, uint8_t* buffer,
                                                     int64_t capacity, int64_t* size) {
  if (size == nullptr || capacity < 0 || n < 0 || (n > 0 && point_data == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  std::vector<uint8_t> payload, msg;
  for (int64_t i = 0; i < n; ++i) wire::put_varint(&payload, static_cast<uint64_t>(static_cast<int64_t>(point_data[i])));
  if (num_points != 0) {
    wire::put_varint(&msg, 1u << 3 | 0);
    wire::put_varint(&msg, static_cast<uint64_t>(static_cast<int64_t>(num_points)));
  }
  wire::put_packed(&msg, 3, payload);
  return deliver(msg, buffer, capacity, size);
}

extern "C" int dliom_compressed_point_cloud_from_proto(const uint8_t* bytes, int64_t size, int32_t* num_points, int32_t* point_data,
                                                       int64_t capacity, int64_t* n) {
  if (num_points == nullptr || n == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_TRY(check_buffer(bytes, size));
  std::vector<int32_t> words;
  DLIOM_TRY(parse_compressed_cloud(bytes, bytes + size, num_points, &words));
  *n = static_cast<int64_t>(words.size());
  if (point_data == nullptr) return DLIOM_OK;  // size query
  if (capacity < *n) return DLIOM_ERR_CAPACITY;
  if (!words.empty()) std::memcpy(point_data, words.data(), 4 * words.size());
  return DLIOM_OK;
}

extern "C" int dliom_compressed_point_cloud_check(int32_t num_points, const int32_t* point_data, int64_t n) {
  std::vector<unsigned> block_first;
  return walk_stream(num_points, point_data, n, &block_first);
}

extern "C" int dliom_cloud_decompress(dliom_ctx* ctx, int32_t num_points, const int32_t* point_data, int64_t n, dliom_cloud** out) {
  if (ctx == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  std::vector<unsigned> block_first;
  DLIOM_TRY(walk_stream(num_points, point_data, n, &block_first));
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  if (num_points == 0) {
    DLIOM_TRY(empty_cloud(ctx, out));
    for (int a = 0; a < 3; ++a) (*out)->abs_max[a] = 0.f;  // known, as an uploaded empty cloud's
    return DLIOM_OK;
  }
  const size_t blocks = block_first.size() - 1;
  const size_t at_first = align256(4 * static_cast<size_t>(n)), at_maxima = at_first + align256(4 * block_first.size());
  DLIOM_TRY(ctx->compress.reserve(at_maxima + 256));
  char* base = static_cast<char*>(ctx->compress.p);
  int32_t* d_stream = reinterpret_cast<int32_t*>(base);
  unsigned *d_first = reinterpret_cast<unsigned*>(base + at_first), *d_maxima = reinterpret_cast<unsigned*>(base + at_maxima);
  DLIOM_HIP_TRY(hipMemcpyAsync(d_stream, point_data, 4 * static_cast<size_t>(n), hipMemcpyHostToDevice, ctx->stream));
  DLIOM_HIP_TRY(hipMemcpyAsync(d_first, block_first.data(), 4 * block_first.size(), hipMemcpyHostToDevice, ctx->stream));
  const FillJob fill{d_maxima, 16, 0u};
  DLIOM_TRY(fill_multi(ctx, &fill, 1));
  float *x, *y, *z;
  DLIOM_TRY(alloc_device_cloud(ctx, num_points, out, &x, &y, &z));
  hipLaunchKernelGGL(decompress_kernel, dim3(blocks_of(num_points, kBlock)), dim3(kBlock), 0, ctx->stream, d_stream, d_first,
                     static_cast<unsigned>(blocks), static_cast<unsigned>(num_points), x, y, z, d_maxima);
  int st = launched() ? DLIOM_OK : DLIOM_ERR_HIP;
  float maxima[4] = {0.f, 0.f, 0.f, 0.f};
  if (st == DLIOM_OK) {
    const GatherJob job{d_maxima, 4};
    unsigned* host = pinned_at<unsigned>(ctx, kPinReadback);
    st = gather_and_wait(ctx, &job, 1, host);
    if (st == DLIOM_OK) std::memcpy(maxima, host, 16);
  }
  if (st == DLIOM_OK) st = finish_device_cloud(ctx, *out, std::sqrt(maxima[0]));  // sqrt is monotone: the max of the norms
  if (st != DLIOM_OK) {
    dliom_cloud_destroy(*out);
    *out = nullptr;
    return st;
  }
  for (int a = 0; a < 3; ++a) (*out)->abs_max[a] = maxima[1 + a];
  return DLIOM_OK;
}

extern "C" int dliom_cloud_from_compressed_proto(dliom_ctx* ctx, const uint8_t* bytes, int64_t size, dliom_cloud** out) {
  if (ctx == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  DLIOM_TRY(check_buffer(bytes, size));
  int32_t num_points = 0;
  std::vector<int32_t> words;
  DLIOM_TRY(parse_compressed_cloud(bytes, bytes + size, &num_points, &words));
  return dliom_cloud_decompress(ctx, num_points, words.data(), static_cast<int64_t>(words.size()), out);
}

extern "C" int dliom_trajectory_nodes_data_to_proto(dliom_ctx* ctx, const dliom_trajectory_node_data* nodes, int count, uint8_t* bytes,
                                                    int64_t capacity, int64_t* byte_offsets, int* first_refused) {
  if (ctx == nullptr || count < 0 || (count > 0 && nodes == nullptr) || byte_offsets == nullptr || first_refused == nullptr ||
      capacity < 0 || count > kMaxBatchClouds / 3)
    return DLIOM_ERR_INVALID_ARGUMENT;
  *first_refused = -1;
  std::vector<const dliom_cloud*> clouds;
  clouds.reserve(3 * static_cast<size_t>(count));
  for (int i = 0; i < count; ++i) {
    if (nodes[i].histogram_size < 0 || (nodes[i].histogram_size > 0 && nodes[i].histogram == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
    clouds.insert(clouds.end(), {nodes[i].filtered_gravity_aligned, nodes[i].high_resolution, nodes[i].low_resolution});
  }
  Batch b;
  DLIOM_TRY(run_batch(ctx, clouds.data(), 3 * count, true, &b));
  if (b.meta[kMetaRefused] != kNoCloud) {
    *first_refused = static_cast<int>(b.meta[kMetaRefused] / 3u);
    return DLIOM_ERR_GRID_EXTENT;
  }
  const uint8_t* payload = nullptr;
  DLIOM_TRY(pack_batch(ctx, b, &payload));
  std::vector<uint8_t> msg, part;
  size_t histogram_bytes = 0;
  for (int i = 0; i < count; ++i) histogram_bytes += 4 * static_cast<size_t>(nodes[i].histogram_size);
  msg.reserve(static_cast<size_t>(b.bytes()) + histogram_bytes + 192 * static_cast<size_t>(count));  // (192: the poses and the framing)
  std::vector<int64_t> ends(static_cast<size_t>(count));
  for (int i = 0; i < count; ++i) {
    const dliom_trajectory_node_data& node = nodes[i];
    if (node.timestamp != 0) {
      wire::put_varint(&msg, 1u << 3 | 0);
      wire::put_varint(&msg, static_cast<uint64_t>(node.timestamp));
    }
    const double* g = node.gravity_alignment_wxyz;  // transform::proto::Quaterniond: x, y, z, w
    part.clear();
    wire::put_double_field(&part, 1, g[1]);
    wire::put_double_field(&part, 2, g[2]);
    wire::put_double_field(&part, 3, g[3]);
    wire::put_double_field(&part, 4, g[0]);
    wire::put_message(&msg, 2, part);
    for (int c = 3 * i; c < 3 * i + 3; ++c) {
      const int64_t payload_bytes = b.byte_off(c + 1) - b.byte_off(c), size = compressed_cloud_size(cloud_points(clouds[c]), payload_bytes);
      wire::put_varint(&msg, static_cast<uint64_t>(3 + c % 3) << 3 | 2);  // always present, even when empty
      wire::put_varint(&msg, static_cast<uint64_t>(size));
      msg.resize(msg.size() + static_cast<size_t>(size));
      put_compressed_cloud(msg.data() + (msg.size() - static_cast<size_t>(size)), cloud_points(clouds[c]), payload + b.byte_off(c), payload_bytes);
    }
    if (node.histogram_size > 0) {  // packed float: every element, zeros too
      wire::put_varint(&msg, 6u << 3 | 2);
      wire::put_varint(&msg, 4 * static_cast<uint64_t>(node.histogram_size));
      const uint8_t* h = reinterpret_cast<const uint8_t*>(node.histogram);
      msg.insert(msg.end(), h, h + 4 * static_cast<size_t>(node.histogram_size));
    }
    wire::put_rigid3d(&msg, 7, node.local_pose7);
    ends[i] = static_cast<int64_t>(msg.size());
  }
  byte_offsets[0] = 0;
  for (int i = 0; i < count; ++i) byte_offsets[i + 1] = ends[i];
  if (bytes == nullptr) return DLIOM_OK;  // size query
  if (capacity < static_cast<int64_t>(msg.size())) return DLIOM_ERR_CAPACITY;
  if (!msg.empty()) std::memcpy(bytes, msg.data(), msg.size());
  return DLIOM_OK;
}

extern "C" int dliom_trajectory_node_data_to_proto(dliom_ctx* ctx, int64_t timestamp, const double gravity_alignment_wxyz[4],
                                                   const dliom_cloud* filtered_gravity_aligned, const dliom_cloud* high_resolution,
                                                   const dliom_cloud* low_resolution, const float* histogram, int histogram_size,
                                                   const double local_pose7[7], uint8_t* buffer, int64_t capacity, int64_t* size) {
  if (gravity_alignment_wxyz == nullptr || local_pose7 == nullptr || size == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_trajectory_node_data node;
  node.timestamp = timestamp;
  std::memcpy(node.gravity_alignment_wxyz, gravity_alignment_wxyz, sizeof node.gravity_alignment_wxyz);
  node.filtered_gravity_aligned = filtered_gravity_aligned;
  node.high_resolution = high_resolution;
  node.low_resolution = low_resolution;
  node.histogram = histogram;
  node.histogram_size = histogram_size;
  std::memcpy(node.local_pose7, local_pose7, sizeof node.local_pose7);
  int64_t offsets[2] = {0, 0};
  int refused = -1;
  const int st = dliom_trajectory_nodes_data_to_proto(ctx, &node, 1, buffer, capacity, offsets, &refused);
  if (st == DLIOM_OK || st == DLIOM_ERR_CAPACITY) *size = offsets[1];
  return st;
}

extern "C" int dliom_trajectory_node_data_from_proto(dliom_ctx* ctx, const uint8_t* bytes, int64_t size, int64_t* timestamp,
                                                     double gravity_alignment_wxyz[4], dliom_cloud** filtered_gravity_aligned,
                                                     dliom_cloud** high_resolution, dliom_cloud** low_resolution, float* histogram,
                                                     int histogram_capacity, int* histogram_size, double local_pose7[7]) {
  if (ctx == nullptr || timestamp == nullptr || gravity_alignment_wxyz == nullptr || filtered_gravity_aligned == nullptr ||
      high_resolution == nullptr || low_resolution == nullptr || histogram_size == nullptr || local_pose7 == nullptr ||
      histogram_capacity < 0 || (histogram_capacity > 0 && histogram == nullptr))
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_TRY(check_buffer(bytes, size));
  dliom_cloud** outs[3] = {filtered_gravity_aligned, high_resolution, low_resolution};
  for (dliom_cloud** o : outs) *o = nullptr;
  *timestamp = 0;
  double q[4] = {0, 0, 0, 0}, t[3] = {0, 0, 0}, r[4] = {0, 0, 0, 0};  // proto3 defaults (x, y, z, w)
  const uint8_t *cloud_at[3] = {nullptr, nullptr, nullptr}, *cloud_end[3] = {nullptr, nullptr, nullptr};
  std::vector<float> hist;
  const uint8_t* p = bytes;
  const uint8_t* end = bytes + size;
  auto take_float = [&](const uint8_t* f) {
    float v;
    std::memcpy(&v, f, 4);
    hist.push_back(v);
  };
  while (p < end) {
    uint64_t tag, v;
    if (!wire::get_varint(p, end, &tag)) return DLIOM_ERR_INVALID_ARGUMENT;
    const unsigned wire_type = static_cast<unsigned>(tag & 7);
    const uint64_t field = tag >> 3;
    if (field == 1 && wire_type == 0) {
      if (!wire::get_varint(p, end, &v)) return DLIOM_ERR_INVALID_ARGUMENT;
      *timestamp = static_cast<int64_t>(v);
    } else if (field == 6 && wire_type == 5) {  // an unpacked element
      if (end - p < 4) return DLIOM_ERR_INVALID_ARGUMENT;
      take_float(p);
      p += 4;
    } else if (wire_type == 2 && (field == 2 || (field >= 3 && field <= 7))) {
      if (!wire::get_varint(p, end, &v) || static_cast<uint64_t>(end - p) < v) return DLIOM_ERR_INVALID_ARGUMENT;
      const uint8_t* e = p + v;
      if (field == 2) {
        if (!wire::parse_doubles(p, e, q, 4)) return DLIOM_ERR_INVALID_ARGUMENT;
      } else if (field <= 5) {  // the last occurrence wins (protobuf would merge; the writers emit one)
        cloud_at[field - 3] = p;
        cloud_end[field - 3] = e;
      } else if (field == 6) {
        if (v % 4 != 0) return DLIOM_ERR_INVALID_ARGUMENT;
        for (const uint8_t* f = p; f < e; f += 4) take_float(f);
      } else {
        if (!wire::parse_rigid3d(p, e, t, r)) return DLIOM_ERR_INVALID_ARGUMENT;
      }
      p = e;
    } else if (!wire::skip_field(p, end, wire_type)) {
      return DLIOM_ERR_INVALID_ARGUMENT;
    }
  }
  *histogram_size = static_cast<int>(hist.size());
  if (histogram_capacity < *histogram_size) return DLIOM_ERR_CAPACITY;
  int st = DLIOM_OK;
  for (int c = 0; c < 3 && st == DLIOM_OK; ++c)
    st = dliom_cloud_from_compressed_proto(ctx, cloud_at[c], cloud_end[c] - cloud_at[c], outs[c]);  // absent: the empty cloud
  if (st != DLIOM_OK) {
    for (dliom_cloud** o : outs) {
      if (*o != nullptr) dliom_cloud_destroy(*o);
      *o = nullptr;
    }
    return st;
  }
  if (!hist.empty()) std::memcpy(histogram, hist.data(), 4 * hist.size());
  gravity_alignment_wxyz[0] = q[3];
  gravity_alignment_wxyz[1] = q[0];
  gravity_alignment_wxyz[2] = q[1];
  gravity_alignment_wxyz[3] = q[2];
  for (int i = 0; i < 3; ++i) local_pose7[i] = t[i];
  local_pose7[3] = r[3];
  local_pose7[4] = r[0];
  local_pose7[5] = r[1];
  local_pose7[6] = r[2];
  return DLIOM_OK;
}
