// Node clouds kept in HBM (dliom.h "node clouds kept in HBM"): every scan's range_data_in_local
// in pooled SoA slabs, and the two per-point loops the D-LIOM fork runs over them as batched device passes.
//   add       one kernel: the filtered cloud (moved by a float pose on the way) into the node's place in a slab
//   pack      PointCloud2 records (x, y, z, 1.0f) of a chunk of nodes in ONE launch: a lane finds its node by bisection
//             of the returns' prefix sums and stores its record as one 16-byte word
//   to_proto  NodeRangeData messages of a chunk of nodes: records of 2 to 17 bytes, placed as points_text.hip places its
//             text -- sizes a tile, a scan, one read-back of the nodes' payload sizes, then an emit pass that stores whole
//             dwords out of LDS and copies the headers the host made
// The descriptor table is the host's; its device mirror is brought up to date by the batched calls.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

#include "device_common.h"
#include "host_math.h"
#include "proto_wire.h"

namespace dliom {
namespace {

constexpr int kBlock = 256;
constexpr int kTile = 256;  // records a tile of the proto passes, one a lane
constexpr int kMaxRecord = DLIOM_NODE_RANGE_MAX_RECORD;
static_assert(kMaxRecord == 2 + 3 * 5, "tag, length, three tagged floats");
constexpr int kStageWords = (3 + kTile * kMaxRecord + 3) / 4;
constexpr int64_t kDefaultSlabFloats = int64_t{1} << 24;
constexpr int64_t kDefaultChunkPoints = int64_t{1} << 22;
constexpr int64_t kMaxNodePoints = (int64_t{1} << 31) - 1;  // returns + misses of a node
constexpr size_t kInitialTableNodes = 1024;

// what a kernel needs of a node: x at p, y at p + stride, z at p + 2 * stride
struct NodeDesc {
  const float* r;
  const float* m;
  unsigned n_r, n_m, stride_r, stride_m;
};

struct Slab {
  float* p = nullptr;
  int64_t cap = 0, used = 0;  // floats
};

int64_t pad16(int64_t n) { return (n + 15) & ~int64_t{15}; }

struct FloatPose {
  Quat4 q;
  float t[3];
};
__host__ __device__ inline FloatPose pose_of(const float* p) { return FloatPose{Quat4{p[3], p[4], p[5], p[6]}, {p[0], p[1], p[2]}}; }
__device__ __forceinline__ void move_point(const FloatPose& p, float& x, float& y, float& z) {
  float rx, ry, rz;
  rotate_point(p.q, x, y, z, rx, ry, rz);
  x = rx + p.t[0];
  y = ry + p.t[1];
  z = rz + p.t[2];
}

struct AddArgs {
  const float *rx, *ry, *rz, *mx, *my, *mz;
  float *dr, *dm;
  unsigned n_r, n_m, stride_r, stride_m;
  int apply;
  FloatPose pose;
};
__global__ __launch_bounds__(kBlock) void node_add_kernel(AddArgs a) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n_r + a.n_m) return;
  const bool ret = i < a.n_r;
  const unsigned j = ret ? i : i - a.n_r;
  float x = ret ? a.rx[j] : a.mx[j], y = ret ? a.ry[j] : a.my[j], z = ret ? a.rz[j] : a.mz[j];
  if (a.apply) move_point(a.pose, x, y, z);
  float* d = ret ? a.dr : a.dm;
  const unsigned stride = ret ? a.stride_r : a.stride_m;
  d[j] = x;
  d[stride + j] = y;
  d[2u * stride + j] = z;
}

__global__ __launch_bounds__(kBlock) void node_interleave_kernel(const float* __restrict__ p, unsigned stride, unsigned n, float* __restrict__ out) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  out[3u * i] = p[i];
  out[3u * i + 1u] = p[stride + i];
  out[3u * i + 2u] = p[2u * stride + i];
}

// the largest c in [lo, hi] with prefix[c] <= g (prefix[lo] <= g): an empty node is never that, unless nothing follows it
__device__ __forceinline__ unsigned node_of(const long long* __restrict__ prefix, unsigned lo, unsigned hi, long long g) {
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo + 1u) >> 1);
    if (prefix[mid] <= g) lo = mid; else hi = mid - 1u;
  }
  return lo;
}

struct PackPoses {
  int num, per_node;
  float shared[14];
  const float* per;  // device: the chunk's first node's poses
};

// Record i of the chunk's nodes [a, b): the workgroup's first and last records bound the nodes its lanes can lie in (one
// node, mostly: no bisection left), a lane bisects the rest.  Loads are a dword a lane from each of the node's three
// arrays, the store is one 16-byte word a lane: a wavefront writes 1 KiB in one instruction.
__global__ __launch_bounds__(kBlock) void node_pack_kernel(const NodeDesc* __restrict__ desc, const long long* __restrict__ ret_prefix,
                                                           unsigned a, unsigned b, unsigned long long n, PackPoses poses,
                                                           float4* __restrict__ out) {
  __shared__ unsigned range[2];
  const long long base = ret_prefix[a];
  const unsigned long long first = static_cast<unsigned long long>(blockIdx.x) * kBlock;
  if (threadIdx.x == 0) range[0] = node_of(ret_prefix, a, b - 1u, base + static_cast<long long>(first));
  if (threadIdx.x == 64) range[1] = node_of(ret_prefix, a, b - 1u, base + static_cast<long long>(min(first + kBlock, n) - 1ull));
  __syncthreads();
  const unsigned long long i = first + threadIdx.x;
  if (i >= n) return;
  const long long g = base + static_cast<long long>(i);
  const unsigned c = node_of(ret_prefix, range[0], range[1], g);
  const NodeDesc d = desc[c];
  const unsigned j = static_cast<unsigned>(g - ret_prefix[c]);
  float x = d.r[j], y = d.r[d.stride_r + j], z = d.r[2u * d.stride_r + j];
  if (poses.num > 0) {
    const float* p = poses.per_node ? poses.per + static_cast<size_t>(c - a) * (7u * poses.num) : poses.shared;
    move_point(pose_of(p), x, y, z);
    if (poses.num > 1) move_point(pose_of(p + 7), x, y, z);
  }
  out[i] = make_float4(x, y, z, 1.0f);
}

__global__ __launch_bounds__(kBlock) void cloud_pack_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, unsigned n, int apply, FloatPose pose,
                                                            float4* __restrict__ out) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float px = x[i], py = y[i], pz = z[i];
  if (apply) move_point(pose, px, py, pz);
  out[i] = make_float4(px, py, pz, 1.0f);
}

// ---- NodeRangeData records ----
struct Record {
  float v[3];
  unsigned tag;     // field 2 (a return) or 3 (a miss), length-delimited
  unsigned length;  // 0: no record (behind the node's last)
};
// v == 0 drops a coordinate: -0.0 is dropped, NaN is written
__device__ __forceinline__ unsigned record_length(const float v[3]) {
  return 2u + 5u * ((v[0] != 0.f ? 1u : 0u) + (v[1] != 0.f ? 1u : 0u) + (v[2] != 0.f ? 1u : 0u));
}
// Tile t of the chunk's nodes [a, b): its node by bisection of the tiles' prefix sums (uniform over the workgroup), then
// the lane's record: the node's returns first, its misses behind them.
__device__ __forceinline__ Record tile_record(const NodeDesc* __restrict__ desc, const long long* __restrict__ tile_prefix, unsigned a,
                                              unsigned b, unsigned t, unsigned* node) {
  const long long gt = tile_prefix[a] + t;
  const unsigned c = node_of(tile_prefix, a, b - 1u, gt);
  *node = c;
  const NodeDesc d = desc[c];
  const unsigned long long j = static_cast<unsigned long long>(gt - tile_prefix[c]) * kTile + threadIdx.x;
  Record r;
  r.v[0] = r.v[1] = r.v[2] = 0.f;
  r.tag = 0u;
  r.length = 0u;
  if (j < static_cast<unsigned long long>(d.n_r) + d.n_m) {
    const bool ret = j < d.n_r;
    const unsigned k = static_cast<unsigned>(ret ? j : j - d.n_r), stride = ret ? d.stride_r : d.stride_m;
    const float* p = ret ? d.r : d.m;
    r.v[0] = p[k];
    r.v[1] = p[stride + k];
    r.v[2] = p[2u * stride + k];
    r.tag = ret ? (2u << 3 | 2u) : (3u << 3 | 2u);
    r.length = record_length(r.v);
  }
  return r;
}

__global__ __launch_bounds__(kTile) void range_size_kernel(const NodeDesc* __restrict__ desc, const long long* __restrict__ tile_prefix,
                                                           unsigned a, unsigned b, unsigned long long* __restrict__ totals) {
  using Reduce = hipcub::BlockReduce<unsigned, kTile>;
  __shared__ typename Reduce::TempStorage temp;
  unsigned node;
  const Record r = tile_record(desc, tile_prefix, a, b, blockIdx.x, &node);
  const unsigned total = Reduce(temp).Sum(r.length);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// bytes of the tiles [0, t) of the chunk
__device__ __forceinline__ unsigned long long bytes_before(const unsigned long long* __restrict__ inclusive, long long t) {
  return t > 0 ? inclusive[t - 1] : 0ull;
}

// One workgroup: the payload bytes of every node of the chunk into page-locked memory, then the completion word.
__global__ __launch_bounds__(kBlock) void range_node_sizes_kernel(const long long* __restrict__ tile_prefix, unsigned a, unsigned b,
                                                                  const unsigned long long* __restrict__ inclusive,
                                                                  unsigned long long* sizes, unsigned* done_word, unsigned done_seq) {
  const long long t_first = tile_prefix[a];
  for (unsigned c = a + threadIdx.x; c < b; c += kBlock)
    sizes[c - a] = bytes_before(inclusive, tile_prefix[c + 1u] - t_first) - bytes_before(inclusive, tile_prefix[c] - t_first);
  if (done_word != nullptr) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence_system();
      *reinterpret_cast<volatile unsigned*>(done_word) = done_seq;
    }
  }
}

// where the host put a node's message in the chunk's bytes, and its header in the blob
struct NodeOut {
  unsigned long long msg_off;
  unsigned hdr_off, hdr_len;
};

// Workgroups [0, tiles): a tile's records, placed in LDS by a scan of their lengths behind the 0 to 3 bytes that align the
// stage with the output's dwords (`out` is 256-byte aligned); whole dwords go out as dwords, the first and the last dword,
// which the neighbours may share, bytewise -- xyz_emit_kernel's scheme.  Workgroups behind them: a node's header a
// wavefront, copied bytewise from the blob the host made.
__global__ __launch_bounds__(kTile) void range_emit_kernel(const NodeDesc* __restrict__ desc, const long long* __restrict__ tile_prefix,
                                                           unsigned a, unsigned b, unsigned tiles,
                                                           const unsigned long long* __restrict__ inclusive,
                                                           const NodeOut* __restrict__ node_out, const unsigned char* __restrict__ blob,
                                                           unsigned char* __restrict__ out) {
  using Scan = hipcub::BlockScan<unsigned, kTile>;
  __shared__ typename Scan::TempStorage temp;
  __shared__ unsigned stage[kStageWords];
  if (blockIdx.x >= tiles) {
    const unsigned c = (blockIdx.x - tiles) * (kTile / 64) + threadIdx.x / 64u;
    if (c >= b - a) return;
    const NodeOut o = node_out[c];
    for (unsigned k = threadIdx.x & 63u; k < o.hdr_len; k += 64u) out[o.msg_off + k] = blob[o.hdr_off + k];
    return;
  }
  unsigned char* bytes = reinterpret_cast<unsigned char*>(stage);
  unsigned c;
  const Record r = tile_record(desc, tile_prefix, a, b, blockIdx.x, &c);
  const NodeOut o = node_out[c - a];
  const long long t_first = tile_prefix[a];
  const unsigned long long before_tile = bytes_before(inclusive, blockIdx.x);
  const unsigned long long first = o.msg_off + o.hdr_len + (before_tile - bytes_before(inclusive, tile_prefix[c] - t_first));
  // (the sizing pass's total: never above kTile * kMaxRecord, which is what the stage holds)
  const unsigned total = static_cast<unsigned>(min(inclusive[blockIdx.x] - before_tile, static_cast<unsigned long long>(kTile * kMaxRecord)));
  const unsigned pad = static_cast<unsigned>(first & 3ull);
  unsigned before;
  Scan(temp).ExclusiveSum(r.length, before);
  if (r.length != 0u && before + r.length <= total) {  // (always: the sizing pass made `total` from the same lengths)
    unsigned char* at = bytes + pad + before;
    at[0] = static_cast<unsigned char>(r.tag);
    at[1] = static_cast<unsigned char>(r.length - 2u);
    at += 2;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      if (r.v[f] != 0.f) {
        const unsigned bits = __float_as_uint(r.v[f]);
        at[0] = static_cast<unsigned char>((f + 1) << 3 | 5);
        at[1] = static_cast<unsigned char>(bits);
        at[2] = static_cast<unsigned char>(bits >> 8);
        at[3] = static_cast<unsigned char>(bits >> 16);
        at[4] = static_cast<unsigned char>(bits >> 24);
        at += 5;
      }
    }
  }
  __syncthreads();
  const unsigned end = pad + total;  // of the range, in stage bytes
  unsigned* out_words = reinterpret_cast<unsigned*>(out + (first - pad));
  unsigned char* out_bytes = out + (first - pad);
  for (unsigned w = threadIdx.x; 4u * w < end; w += kTile) {
    if (4u * w >= pad && 4u * w + 4u <= end) {
      out_words[w] = stage[w];
    } else {
      for (unsigned k = 4u * w; k < 4u * w + 4u; ++k)
        if (k >= pad && k < end) out_bytes[k] = bytes[k];
    }
  }
}

bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace
}  // namespace dliom

using namespace dliom;

struct dliom_node_clouds {
  dliom_ctx* ctx = nullptr;
  int64_t slab_floats = kDefaultSlabFloats;
  std::vector<Slab> slabs;
  std::vector<NodeDesc> desc;  // the descriptor table: a node each, and the prefix sums (nodes + 1 each)
  std::vector<dliom_node_cloud_info> info;
  std::vector<long long> ret_prefix{0}, item_prefix{0}, tile_prefix{0};
  // the device mirror: [desc | ret_prefix | tile_prefix] for table_nodes nodes, the first `mirrored` of them current
  DevBuf d_table;
  size_t table_nodes = 0;
  int64_t mirrored = 0;
  DevBuf work, poses;
  int64_t nodes() const { return static_cast<int64_t>(desc.size()); }
  const NodeDesc* d_desc() const { return d_table.as<NodeDesc>(); }
  const long long* d_ret_prefix() const { return reinterpret_cast<const long long*>(d_table.as<char>() + align256(sizeof(NodeDesc) * table_nodes)); }
  const long long* d_tile_prefix() const { return d_ret_prefix() + align256(8 * (table_nodes + 1)) / 8; }
};

namespace dliom {
namespace {

// floats for a node: in the open slab, else in a new one (a node larger than a slab gets one of its own size)
int slab_take(dliom_node_clouds* nc, int64_t need, float** out) {
  if (need == 0) {
    *out = nullptr;
    return DLIOM_OK;
  }
  if (!nc->slabs.empty() && nc->slabs.back().cap - nc->slabs.back().used >= need) {
    Slab& s = nc->slabs.back();
    *out = s.p + s.used;
    s.used += need;
    return DLIOM_OK;
  }
  Slab s;
  s.cap = std::max(need, nc->slab_floats);
  void* p = nullptr;
  DLIOM_HIP_TRY(hipMalloc(&p, 4 * static_cast<size_t>(s.cap)));
  s.p = static_cast<float*>(p);
  s.used = need;
  *out = s.p;
  // the open slab is the last one: a dedicated slab goes in front of it, so that the open one keeps filling
  if (need > nc->slab_floats && !nc->slabs.empty()) nc->slabs.insert(nc->slabs.end() - 1, s);
  else nc->slabs.push_back(s);
  return DLIOM_OK;
}

// Brings the device mirror up to date with the host's table; waits for its copies, since the host table may grow next.
int mirror_table(dliom_node_clouds* nc) {
  const int64_t n = nc->nodes();
  if (nc->mirrored == n && nc->d_table.p != nullptr) return DLIOM_OK;
  dliom_ctx* ctx = nc->ctx;
  if (static_cast<size_t>(n) > nc->table_nodes || nc->d_table.p == nullptr) {
    const size_t want = std::max({static_cast<size_t>(n), 2 * nc->table_nodes, kInitialTableNodes});
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // nothing may still read the old mirror
    DLIOM_TRY(nc->d_table.reserve(align256(sizeof(NodeDesc) * want) + 2 * align256(8 * (want + 1))));
    nc->table_nodes = want;
    nc->mirrored = 0;
  }
  const size_t from = static_cast<size_t>(nc->mirrored), fresh = static_cast<size_t>(n) - from;
  if (fresh > 0)
    DLIOM_HIP_TRY(hipMemcpyAsync(const_cast<NodeDesc*>(nc->d_desc()) + from, nc->desc.data() + from, sizeof(NodeDesc) * fresh,
                                 hipMemcpyHostToDevice, ctx->stream));
  // (the entry behind the last node is the total: rewritten when a node takes its place)
  DLIOM_HIP_TRY(hipMemcpyAsync(const_cast<long long*>(nc->d_ret_prefix()) + from, nc->ret_prefix.data() + from, 8 * (fresh + 1),
                               hipMemcpyHostToDevice, ctx->stream));
  DLIOM_HIP_TRY(hipMemcpyAsync(const_cast<long long*>(nc->d_tile_prefix()) + from, nc->tile_prefix.data() + from, 8 * (fresh + 1),
                               hipMemcpyHostToDevice, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  nc->mirrored = n;
  return DLIOM_OK;
}

int check_range(const dliom_node_clouds* nc, int64_t first, int64_t count) {
  return nc == nullptr || first < 0 || count < 0 || first > nc->nodes() || count > nc->nodes() - first ? DLIOM_ERR_INVALID_ARGUMENT : DLIOM_OK;
}

// Whole nodes, up to `most` of what `prefix` sums a chunk, but at least one node that is not empty: empty nodes ride along
// with the chunk in front of them (the leading ones with the first), so every chunk runs the same launches (only a call whose nodes are all empty has a chunk with nothing to size).
std::vector<std::pair<int64_t, int64_t>> plan_chunks(const std::vector<long long>& prefix, int64_t first, int64_t count, int64_t most) {
  std::vector<std::pair<int64_t, int64_t>> chunks;
  int64_t a = first;
  const int64_t end = first + count;
  while (a < end) {
    int64_t b = a + 1;
    while (b < end && (prefix[b + 1] - prefix[a] <= most || prefix[b] == prefix[a] || prefix[b + 1] == prefix[b])) ++b;
    chunks.emplace_back(a, b);
    a = b;
  }
  return chunks;
}

int64_t chunk_limit(const dliom_node_clouds_limits* limits) {
  return limits != nullptr && limits->max_points_per_chunk > 0 ? limits->max_points_per_chunk : kDefaultChunkPoints;
}

// The stream may still read host memory of this call (a pose upload, a header blob): no way out without waiting.
int finish(dliom_ctx* ctx, int status) {
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && status == DLIOM_OK) status = DLIOM_ERR_HIP;
  ++ctx->host_syncs;
  return status;
}

int pack_nodes(dliom_node_clouds* nc, int64_t first, int64_t count, const dliom_node_clouds_transform* transform,
               const dliom_node_clouds_limits* limits, uint8_t* bytes, dliom_node_clouds_stats* stats) {
  dliom_ctx* ctx = nc->ctx;
  DLIOM_TRY(mirror_table(nc));
  PackPoses poses{};
  if (transform != nullptr && transform->num_poses > 0) {
    poses.num = transform->num_poses;
    poses.per_node = transform->per_node;
    if (poses.per_node) {
      const size_t pose_bytes = 28 * static_cast<size_t>(poses.num) * static_cast<size_t>(count);
      DLIOM_TRY(nc->poses.reserve(pose_bytes));
      DLIOM_HIP_TRY(hipMemcpyAsync(nc->poses.p, transform->poses7, pose_bytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
      std::memcpy(poses.shared, transform->poses7, 28 * static_cast<size_t>(poses.num));
    }
  }
  const auto chunks = plan_chunks(nc->ret_prefix, first, count, chunk_limit(limits));
  long long most = 0;
  for (const auto& ch : chunks) most = std::max(most, nc->ret_prefix[ch.second] - nc->ret_prefix[ch.first]);
  DLIOM_TRY(nc->work.reserve(16 * static_cast<size_t>(most)));
  for (const auto& ch : chunks) {
    const long long n = nc->ret_prefix[ch.second] - nc->ret_prefix[ch.first];
    if (n == 0) continue;
    if (poses.per_node) poses.per = nc->poses.as<float>() + static_cast<size_t>(ch.first - first) * 7 * static_cast<size_t>(poses.num);
    hipLaunchKernelGGL(node_pack_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, ctx->stream, nc->d_desc(), nc->d_ret_prefix(),
                       static_cast<unsigned>(ch.first), static_cast<unsigned>(ch.second), static_cast<unsigned long long>(n), poses,
                       nc->work.as<float4>());
    if (!launched()) return DLIOM_ERR_HIP;
    // (in stream order: the next chunk's launch writes the buffer only after this copy has read it)
    DLIOM_HIP_TRY(hipMemcpyAsync(bytes + 16 * (nc->ret_prefix[ch.first] - nc->ret_prefix[first]), nc->work.p, 16 * static_cast<size_t>(n),
                                 hipMemcpyDeviceToHost, ctx->stream));
    if (stats != nullptr) {
      ++stats->chunks;
      ++stats->launches;
    }
  }
  return DLIOM_OK;
}

uint8_t* put_varint_at(uint8_t* out, uint64_t v) {
  while (v >= 0x80) {
    *out++ = static_cast<uint8_t>(v) | 0x80;
    v >>= 7;
  }
  *out++ = static_cast<uint8_t>(v);
  return out;
}

// A node's bytes in front of its records: fields 1 to 4, field 5's tag and length, the origin.  `payload`: the records' bytes.
void put_header(std::vector<uint8_t>* out, const dliom_node_cloud_info& info, uint64_t payload) {
  if (info.timestamp != 0) {
    wire::put_varint(out, 1u << 3 | 0);
    wire::put_varint(out, static_cast<uint64_t>(info.timestamp));
  }
  if (info.trajectory_id != 0) {
    wire::put_varint(out, 2u << 3 | 0);
    wire::put_varint(out, static_cast<uint64_t>(static_cast<int64_t>(info.trajectory_id)));
  }
  if (info.node_index != 0) {
    wire::put_varint(out, 3u << 3 | 0);
    wire::put_varint(out, static_cast<uint64_t>(static_cast<int64_t>(info.node_index)));
  }
  wire::put_rigid3d(out, 4, info.local_pose7);
  std::vector<uint8_t> origin;
  wire::put_vector3f(&origin, 1, info.origin_in_local);
  wire::put_varint(out, 5u << 3 | 2);
  wire::put_varint(out, origin.size() + payload);
  out->insert(out->end(), origin.begin(), origin.end());
}

// The chunk's scratch in nc->work: totals | inclusive | hipcub's | node_out | blob | the bytes
struct ProtoScratch {
  unsigned long long *totals, *inclusive;
  void* tmp;
  size_t tmp_bytes;
  NodeOut* node_out;  // k entries, the blob right behind them
  size_t upload_room;
  unsigned char* out;
};
constexpr size_t kMaxHeader = DLIOM_NODE_RANGE_MAX_HEADER;  // 11 + 11 + 11 + 71 (the pose) + 11 + 17 (the origin), rounded up

size_t proto_scratch_bytes(dliom_ctx* ctx, int64_t tiles, int64_t k, long long items, bool with_bytes, ProtoScratch* s, char* base, int* status) {
  size_t tmp = 0;
  *status = DLIOM_OK;
  if (hipcub::DeviceScan::InclusiveSum(nullptr, tmp, static_cast<const unsigned long long*>(nullptr), static_cast<unsigned long long*>(nullptr),
                                       static_cast<int>(std::max<int64_t>(tiles, 1)), ctx->stream) != hipSuccess)
    *status = DLIOM_ERR_HIP;
  const size_t per = align256(8 * static_cast<size_t>(std::max<int64_t>(tiles, 1)));
  const size_t upload = align256((sizeof(NodeOut) + kMaxHeader) * static_cast<size_t>(k));
  const size_t at_out = 2 * per + align256(tmp) + upload;
  if (s != nullptr) {
    s->totals = reinterpret_cast<unsigned long long*>(base);
    s->inclusive = reinterpret_cast<unsigned long long*>(base + per);
    s->tmp = base + 2 * per;
    s->tmp_bytes = tmp;
    s->node_out = reinterpret_cast<NodeOut*>(base + 2 * per + align256(tmp));
    s->upload_room = upload;
    s->out = reinterpret_cast<unsigned char*>(base + at_out);
  }
  return at_out + (with_bytes ? align256(kMaxHeader * static_cast<size_t>(k) + kMaxRecord * static_cast<size_t>(items)) : 0);
}

// where a chunk's messages go instead of the host: through gzip.hip, a framed record each (dliom_node_clouds_to_pbstream)
struct GzipSink {
  uint8_t* out;
  int64_t capacity;
  int64_t* offsets;  // count + 1, of the records
  dliom_gzip_stats* stats;
  int64_t nodes_done = 0;
  bool fits = true;
};

// sink != nullptr: `bytes` and `capacity` are not used, byte_offsets are still the messages' (uncompressed) offsets
int protos_of_nodes(dliom_node_clouds* nc, int64_t first, int64_t count, const dliom_node_clouds_limits* limits, uint8_t* bytes,
                    int64_t capacity, int64_t* byte_offsets, dliom_node_clouds_stats* stats, bool* fits, GzipSink* sink = nullptr) {
  dliom_ctx* ctx = nc->ctx;
  const bool want_bytes = bytes != nullptr || sink != nullptr;
  DLIOM_TRY(mirror_table(nc));
  const auto chunks = plan_chunks(nc->item_prefix, first, count, chunk_limit(limits));
  size_t most = 0;
  for (const auto& ch : chunks) {
    int st;
    most = std::max(most, proto_scratch_bytes(ctx, nc->tile_prefix[ch.second] - nc->tile_prefix[ch.first], ch.second - ch.first,
                                              nc->item_prefix[ch.second] - nc->item_prefix[ch.first], want_bytes, nullptr, nullptr, &st));
    DLIOM_TRY(st);
  }
  DLIOM_TRY(nc->work.reserve(most));
  std::vector<std::vector<uint8_t>> uploads;  // alive until the call's last wait
  uploads.reserve(chunks.size());
  std::vector<uint8_t> header;
  int64_t at = 0;  // of the chunk's first byte in the call's bytes
  *fits = true;
  for (const auto& ch : chunks) {
    const unsigned a = static_cast<unsigned>(ch.first), b = static_cast<unsigned>(ch.second), k = b - a;
    const long long tiles = nc->tile_prefix[b] - nc->tile_prefix[a], items = nc->item_prefix[b] - nc->item_prefix[a];
    ProtoScratch s;
    int st;
    proto_scratch_bytes(ctx, tiles, k, items, want_bytes, &s, nc->work.as<char>(), &st);
    DLIOM_TRY(st);
    const unsigned long long* sizes = nullptr;
    if (tiles > 0) {
      hipLaunchKernelGGL(range_size_kernel, dim3(static_cast<unsigned>(tiles)), dim3(kTile), 0, ctx->stream, nc->d_desc(), nc->d_tile_prefix(), a, b,
                         s.totals);
      if (!launched()) return DLIOM_ERR_HIP;
      size_t tmp = s.tmp_bytes;
      DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(s.tmp, tmp, s.totals, s.inclusive, static_cast<int>(tiles), ctx->stream));
      DLIOM_TRY(ctx->reserve_batch_pinned(8 * static_cast<size_t>(k)));
      unsigned long long* pinned = static_cast<unsigned long long*>(ctx->batch_pinned);
      const unsigned seq = ctx->done_word != nullptr ? next_done_seq(ctx) : 0u;
      hipLaunchKernelGGL(range_node_sizes_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, nc->d_tile_prefix(), a, b, s.inclusive, pinned,
                         ctx->done_word, seq);
      if (!launched()) return DLIOM_ERR_HIP;
      if (ctx->done_word != nullptr) {
        DLIOM_TRY(wait_done(ctx, ctx->stream, ctx->done_word, seq, 150 + static_cast<int>(std::min<long long>(items / 10000, 100000))));
      } else {
        DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
      }
      sizes = pinned;
      if (stats != nullptr) {
        stats->launches += 3;
        ++stats->readbacks;
      }
    }
    // the headers, and where every message lies
    uploads.emplace_back();
    std::vector<uint8_t>& up = uploads.back();
    up.resize(sizeof(NodeOut) * k);
    int64_t chunk_bytes = 0;
    for (unsigned c = 0; c < k; ++c) {
      const uint64_t payload = sizes != nullptr ? sizes[c] : 0u;
      header.clear();
      put_header(&header, nc->info[a + c], payload);
      NodeOut o;
      o.msg_off = static_cast<unsigned long long>(chunk_bytes);
      o.hdr_off = static_cast<unsigned>(up.size() - sizeof(NodeOut) * k);
      o.hdr_len = static_cast<unsigned>(header.size());
      std::memcpy(up.data() + sizeof(NodeOut) * c, &o, sizeof o);
      up.insert(up.end(), header.begin(), header.end());
      byte_offsets[a - first + c] = at + chunk_bytes;
      chunk_bytes += static_cast<int64_t>(header.size() + payload);
    }
    byte_offsets[b - first] = at + chunk_bytes;
    if (stats != nullptr) ++stats->chunks;
    if (sink == nullptr && bytes != nullptr && *fits && at + chunk_bytes > capacity) *fits = false;  // the sizes of the rest are still owed
    if (want_bytes && *fits && chunk_bytes > 0) {
      if (up.size() > s.upload_room) return DLIOM_ERR_INTERNAL;
      DLIOM_HIP_TRY(hipMemcpyAsync(s.node_out, up.data(), up.size(), hipMemcpyHostToDevice, ctx->stream));
      hipLaunchKernelGGL(range_emit_kernel, dim3(static_cast<unsigned>(tiles) + blocks_of(k, kTile / 64)), dim3(kTile), 0, ctx->stream, nc->d_desc(),
                         nc->d_tile_prefix(), a, b, static_cast<unsigned>(tiles), s.inclusive, s.node_out,
                         reinterpret_cast<const unsigned char*>(s.node_out + k), s.out);
      if (!launched()) return DLIOM_ERR_HIP;
      if (stats != nullptr) ++stats->launches;
      if (sink == nullptr) {
        DLIOM_HIP_TRY(hipMemcpyAsync(bytes + at, s.out, static_cast<size_t>(chunk_bytes), hipMemcpyDeviceToHost, ctx->stream));
      } else {
        // the chunk's messages as segments of s.out; the records behind those of the chunks before (a chunk that does not
        // fit, and every chunk behind it, still runs: the records' sizes are owed, their bytes are not)
        std::vector<int64_t> segments(k + 1u);
        for (unsigned c = 0; c <= k; ++c) segments[c] = byte_offsets[a - first + c] - at;
        int64_t* record = sink->offsets + sink->nodes_done;
        const int64_t gz_at = sink->nodes_done == 0 ? 0 : record[0];
        const int64_t room = sink->fits ? sink->capacity - gz_at : 0;
        const int st = gzip_on_device(ctx, s.out, segments.data(), k, true, sink->out + (sink->fits ? gz_at : 0), room, record, sink->stats);
        if (st == DLIOM_ERR_CAPACITY) sink->fits = false;
        else if (st != DLIOM_OK) return st;
        for (unsigned c = 1; c <= k; ++c) record[c] += gz_at;
        record[0] = gz_at;
        sink->nodes_done += k;
      }
    }
    at += chunk_bytes;
  }
  if (count == 0) byte_offsets[0] = 0;
  return DLIOM_OK;
}

void clear_stats(dliom_node_clouds_stats* stats) {
  if (stats != nullptr) *stats = dliom_node_clouds_stats{0, 0, 0, 0, 0};
}

int download_part(dliom_node_clouds* nc, const float* p, unsigned stride, unsigned n, float* xyz) {
  if (n == 0 || xyz == nullptr) return DLIOM_OK;
  dliom_ctx* ctx = nc->ctx;
  DLIOM_TRY(nc->work.reserve(12 * static_cast<size_t>(n)));
  hipLaunchKernelGGL(node_interleave_kernel, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, ctx->stream, p, stride, n, nc->work.as<float>());
  if (!launched()) return DLIOM_ERR_HIP;
  DLIOM_HIP_TRY(hipMemcpyAsync(xyz, nc->work.p, 12 * static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  return DLIOM_OK;
}

void release_slabs(dliom_node_clouds* nc, size_t keep) {
  while (nc->slabs.size() > keep) {
    (void)hipFree(nc->slabs.back().p);
    nc->slabs.pop_back();
  }
}

// sensor::proto::RangeData: 1 origin, 2 returns, 3 misses; a second occurrence of the message merges into the first
bool parse_range_data(const uint8_t* p, const uint8_t* end, float origin[3], std::vector<float>* returns, std::vector<float>* misses) {
  while (p < end) {
    uint64_t tag, len;
    if (!wire::get_varint(p, end, &tag) || (tag >> 3) == 0) return false;
    const unsigned wire_type = static_cast<unsigned>(tag & 7);
    const uint64_t field = tag >> 3;
    if (wire_type == 2 && field >= 1 && field <= 3) {
      if (!wire::get_varint(p, end, &len) || static_cast<uint64_t>(end - p) < len) return false;
      if (field == 1) {
        if (!wire::parse_floats(p, p + len, origin, 3)) return false;
      } else {
        float v[3] = {0.f, 0.f, 0.f};
        if (!wire::parse_floats(p, p + len, v, 3)) return false;
        std::vector<float>* to = field == 2 ? returns : misses;
        to->insert(to->end(), v, v + 3);
      }
      p += len;
    } else if (!wire::skip_field(p, end, wire_type)) {
      return false;
    }
  }
  return true;
}

// mapping::proto::NodeRangeData: absent fields zero, unknown fields skipped
bool parse_node_range_data(const uint8_t* p, const uint8_t* end, dliom_node_cloud_info* parsed, std::vector<float>* ret, std::vector<float>* mis) {
  std::memset(parsed, 0, sizeof *parsed);
  double t[3] = {0, 0, 0}, q[4] = {0, 0, 0, 0};  // proto3 defaults (x, y, z, w)
  while (p < end) {
    uint64_t tag, v;
    if (!wire::get_varint(p, end, &tag) || (tag >> 3) == 0) return false;
    const unsigned wire_type = static_cast<unsigned>(tag & 7);
    const uint64_t field = tag >> 3;
    if (wire_type == 0 && field >= 1 && field <= 3) {
      if (!wire::get_varint(p, end, &v)) return false;
      if (field == 1) parsed->timestamp = static_cast<int64_t>(v);
      else if (field == 2) parsed->trajectory_id = static_cast<int32_t>(v);
      else parsed->node_index = static_cast<int32_t>(v);
    } else if (wire_type == 2 && (field == 4 || field == 5)) {
      if (!wire::get_varint(p, end, &v) || static_cast<uint64_t>(end - p) < v) return false;
      const bool ok = field == 4 ? wire::parse_rigid3d(p, p + v, t, q) : parse_range_data(p, p + v, parsed->origin_in_local, ret, mis);
      if (!ok) return false;
      p += v;
    } else if (!wire::skip_field(p, end, wire_type)) {
      return false;
    }
  }
  for (int i = 0; i < 3; ++i) parsed->local_pose7[i] = t[i];
  parsed->local_pose7[3] = q[3];
  parsed->local_pose7[4] = q[0];
  parsed->local_pose7[5] = q[1];
  parsed->local_pose7[6] = q[2];
  return true;
}

}  // namespace
}  // namespace dliom

extern "C" {

int dliom_node_clouds_create_sized(dliom_ctx* ctx, int64_t slab_floats, dliom_node_clouds** out) {
  if (ctx == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_node_clouds* nc = new dliom_node_clouds;
  nc->ctx = ctx;
  nc->slab_floats = slab_floats > 0 ? pad16(slab_floats) : kDefaultSlabFloats;
  *out = nc;
  return DLIOM_OK;
}

int dliom_node_clouds_create(dliom_ctx* ctx, dliom_node_clouds** out) { return dliom_node_clouds_create_sized(ctx, 0, out); }

int dliom_node_clouds_destroy(dliom_node_clouds* nc) {
  if (nc == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  (void)hipSetDevice(nc->ctx->device);
  (void)hipStreamSynchronize(nc->ctx->stream);
  release_slabs(nc, 0);
  nc->d_table.release();
  nc->work.release();
  nc->poses.release();
  delete nc;
  return DLIOM_OK;
}

int dliom_node_clouds_clear(dliom_node_clouds* nc) {
  if (nc == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(nc->ctx->device));
  DLIOM_HIP_TRY(hipStreamSynchronize(nc->ctx->stream));  // an add may still write, a download may still read
  release_slabs(nc, 1);
  if (!nc->slabs.empty()) nc->slabs[0].used = 0;
  nc->desc.clear();
  nc->info.clear();
  nc->ret_prefix.assign(1, 0);
  nc->item_prefix.assign(1, 0);
  nc->tile_prefix.assign(1, 0);
  nc->mirrored = 0;
  return DLIOM_OK;
}

int dliom_node_clouds_add(dliom_node_clouds* nc, const dliom_node_cloud_info* info, const dliom_cloud* returns, const dliom_cloud* misses,
                          const float pose_to_local[7], int64_t* index) {
  if (nc == nullptr || info == nullptr || returns == nullptr || returns->ctx != nc->ctx || (misses != nullptr && misses->ctx != nc->ctx))
    return DLIOM_ERR_INVALID_ARGUMENT;
  const int64_t n_r = returns->n, n_m = misses != nullptr ? misses->n : 0;
  if (n_r < 0 || n_m < 0 || n_r + n_m > kMaxNodePoints) return DLIOM_ERR_TOO_LARGE;
  dliom_ctx* ctx = nc->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const int64_t stride_r = pad16(n_r), stride_m = pad16(n_m);
  float* base = nullptr;
  DLIOM_TRY(slab_take(nc, 3 * (stride_r + stride_m), &base));
  NodeDesc d;
  d.r = base;
  d.m = base != nullptr ? base + 3 * stride_r : nullptr;
  d.n_r = static_cast<unsigned>(n_r);
  d.n_m = static_cast<unsigned>(n_m);
  d.stride_r = static_cast<unsigned>(stride_r);
  d.stride_m = static_cast<unsigned>(stride_m);
  if (n_r + n_m > 0) {
    AddArgs a;
    a.rx = returns->d_x;
    a.ry = returns->d_y;
    a.rz = returns->d_z;
    a.mx = misses != nullptr ? misses->d_x : nullptr;
    a.my = misses != nullptr ? misses->d_y : nullptr;
    a.mz = misses != nullptr ? misses->d_z : nullptr;
    a.dr = base;
    a.dm = base + 3 * stride_r;
    a.n_r = d.n_r;
    a.n_m = d.n_m;
    a.stride_r = d.stride_r;
    a.stride_m = d.stride_m;
    a.apply = pose_to_local != nullptr ? 1 : 0;
    const float identity[7] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    a.pose = pose_of(pose_to_local != nullptr ? pose_to_local : identity);
    hipLaunchKernelGGL(node_add_kernel, dim3(blocks_of(n_r + n_m, kBlock)), dim3(kBlock), 0, ctx->stream, a);
    if (!launched()) return DLIOM_ERR_HIP;  // (the floats taken from the slab stay taken: no node names them)
  }
  if (index != nullptr) *index = nc->nodes();
  nc->desc.push_back(d);
  nc->info.push_back(*info);
  nc->ret_prefix.push_back(nc->ret_prefix.back() + n_r);
  nc->item_prefix.push_back(nc->item_prefix.back() + n_r + n_m);
  nc->tile_prefix.push_back(nc->tile_prefix.back() + (n_r + n_m + kTile - 1) / kTile);
  return DLIOM_OK;
}

int dliom_node_clouds_size(const dliom_node_clouds* nc, int64_t* nodes, int64_t* returns, int64_t* misses) {
  if (nc == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (nodes != nullptr) *nodes = nc->nodes();
  if (returns != nullptr) *returns = nc->ret_prefix.back();
  if (misses != nullptr) *misses = nc->item_prefix.back() - nc->ret_prefix.back();
  return DLIOM_OK;
}

int dliom_node_clouds_info(const dliom_node_clouds* nc, int64_t index, dliom_node_cloud_info* info, int64_t* num_returns, int64_t* num_misses) {
  if (nc == nullptr || index < 0 || index >= nc->nodes()) return DLIOM_ERR_INVALID_ARGUMENT;
  if (info != nullptr) *info = nc->info[index];
  if (num_returns != nullptr) *num_returns = nc->desc[index].n_r;
  if (num_misses != nullptr) *num_misses = nc->desc[index].n_m;
  return DLIOM_OK;
}

int dliom_node_clouds_memory_stats(const dliom_node_clouds* nc, dliom_node_clouds_memory* memory) {
  if (nc == nullptr || memory == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *memory = dliom_node_clouds_memory{0, 0, 0, 0, 0};
  memory->slabs = static_cast<int64_t>(nc->slabs.size());
  for (const Slab& s : nc->slabs) {
    memory->bytes_used += 4 * s.used;
    memory->bytes_reserved += 4 * s.cap;
  }
  memory->table_bytes = static_cast<int64_t>(nc->d_table.cap);
  memory->scratch_bytes = static_cast<int64_t>(nc->work.cap + nc->poses.cap);
  return DLIOM_OK;
}

int dliom_node_clouds_download(const dliom_node_clouds* nc_const, int64_t index, float* returns_xyz, float* misses_xyz) {
  if (nc_const == nullptr || index < 0 || index >= nc_const->nodes()) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_node_clouds* nc = const_cast<dliom_node_clouds*>(nc_const);  // (the work buffer is a cache of nothing)
  DLIOM_HIP_TRY(hipSetDevice(nc->ctx->device));
  const NodeDesc& d = nc->desc[index];
  DLIOM_TRY(download_part(nc, d.r, d.stride_r, d.n_r, returns_xyz));
  return download_part(nc, d.m, d.stride_m, d.n_m, misses_xyz);
}

int dliom_node_clouds_pack_point_cloud2(dliom_node_clouds* nc, int64_t first, int64_t count, const dliom_node_clouds_transform* transform,
                                        const dliom_node_clouds_limits* limits, uint8_t* bytes, int64_t capacity, int64_t* byte_offsets,
                                        dliom_node_clouds_stats* stats) {
  if (byte_offsets == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_TRY(check_range(nc, first, count));
  if (transform != nullptr &&
      (transform->num_poses < 0 || transform->num_poses > 2 || (transform->per_node != 0 && transform->per_node != 1) ||
       (transform->num_poses > 0 && transform->poses7 == nullptr && (count > 0 || transform->per_node == 0))))
    return DLIOM_ERR_INVALID_ARGUMENT;
  clear_stats(stats);
  for (int64_t i = 0; i <= count; ++i) byte_offsets[i] = 16 * (nc->ret_prefix[first + i] - nc->ret_prefix[first]);
  const int64_t total = byte_offsets[count];
  if (stats != nullptr) {
    stats->points = total / 16;
    stats->bytes = total;
  }
  if (bytes == nullptr) return DLIOM_OK;  // size query
  if (capacity < total) return DLIOM_ERR_CAPACITY;
  if (total == 0) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(nc->ctx->device));
  return finish(nc->ctx, pack_nodes(nc, first, count, transform, limits, bytes, stats));
}

int dliom_cloud_pack_point_cloud2(const dliom_cloud* cloud, const float pose[7], uint8_t* bytes, int64_t capacity, int64_t* num_bytes) {
  if (cloud == nullptr || num_bytes == nullptr || capacity < 0 || cloud->n > INT32_MAX) return DLIOM_ERR_INVALID_ARGUMENT;
  *num_bytes = 16 * cloud->n;
  if (bytes == nullptr) return DLIOM_OK;
  if (capacity < *num_bytes) return DLIOM_ERR_CAPACITY;
  if (cloud->n == 0) return DLIOM_OK;
  dliom_ctx* ctx = cloud->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(ctx->compress_out.reserve(static_cast<size_t>(*num_bytes)));
  const float identity[7] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
  hipLaunchKernelGGL(cloud_pack_kernel, dim3(blocks_of(cloud->n, kBlock)), dim3(kBlock), 0, ctx->stream, cloud->d_x, cloud->d_y, cloud->d_z,
                     static_cast<unsigned>(cloud->n), pose != nullptr ? 1 : 0, pose_of(pose != nullptr ? pose : identity),
                     ctx->compress_out.as<float4>());
  if (!launched()) return DLIOM_ERR_HIP;
  DLIOM_HIP_TRY(hipMemcpyAsync(bytes, ctx->compress_out.p, static_cast<size_t>(*num_bytes), hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  return DLIOM_OK;
}

int dliom_rigid3f_inverse(const float pose[7], float inverse[7]) {
  if (pose == nullptr || inverse == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  const QF conjugate{pose[3], -pose[4], -pose[5], -pose[6]};
  const F3 t = qrot(conjugate, F3{pose[0], pose[1], pose[2]});
  inverse[0] = -t.x;
  inverse[1] = -t.y;
  inverse[2] = -t.z;
  inverse[3] = conjugate.w;
  inverse[4] = conjugate.x;
  inverse[5] = conjugate.y;
  inverse[6] = conjugate.z;
  return DLIOM_OK;
}

int dliom_node_clouds_to_proto(dliom_node_clouds* nc, int64_t first, int64_t count, const dliom_node_clouds_limits* limits, uint8_t* bytes,
                               int64_t capacity, int64_t* byte_offsets, dliom_node_clouds_stats* stats) {
  if (byte_offsets == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_TRY(check_range(nc, first, count));
  clear_stats(stats);
  byte_offsets[0] = 0;
  if (count == 0) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(nc->ctx->device));
  bool fits = true;
  const int st = finish(nc->ctx, protos_of_nodes(nc, first, count, limits, bytes, capacity, byte_offsets, stats, &fits));
  if (st != DLIOM_OK) return st;
  if (stats != nullptr) {
    stats->points = nc->item_prefix[first + count] - nc->item_prefix[first];
    stats->bytes = byte_offsets[count];
  }
  return fits ? DLIOM_OK : DLIOM_ERR_CAPACITY;
}

int dliom_node_clouds_to_pbstream(dliom_node_clouds* nc, int64_t first, int64_t count, const dliom_node_clouds_limits* limits, uint8_t* bytes,
                                  int64_t capacity, int64_t* byte_offsets, dliom_node_clouds_stats* stats, dliom_gzip_stats* gzip_stats) {
  if (bytes == nullptr || byte_offsets == nullptr || capacity < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_TRY(check_range(nc, first, count));
  clear_stats(stats);
  if (gzip_stats != nullptr) *gzip_stats = dliom_gzip_stats{0, 0, 0, 0};
  byte_offsets[0] = 0;
  if (count == 0) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(nc->ctx->device));
  std::vector<int64_t> message_offsets(static_cast<size_t>(count) + 1);
  GzipSink sink{bytes, capacity, byte_offsets, gzip_stats};
  bool fits = true;
  const int st = finish(nc->ctx, protos_of_nodes(nc, first, count, limits, nullptr, 0, message_offsets.data(), stats, &fits, &sink));
  if (st != DLIOM_OK) return st;
  if (stats != nullptr) {
    stats->points = nc->item_prefix[first + count] - nc->item_prefix[first];
    stats->bytes = byte_offsets[count];
  }
  return sink.fits ? DLIOM_OK : DLIOM_ERR_CAPACITY;
}

int dliom_node_range_data_check(const uint8_t* bytes, int64_t size, dliom_node_cloud_info* info, int64_t* num_returns, int64_t* num_misses) {
  if (size < 0 || (size > 0 && bytes == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_node_cloud_info parsed;
  std::vector<float> ret, mis;
  if (!parse_node_range_data(bytes, bytes + size, &parsed, &ret, &mis)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (info != nullptr) *info = parsed;
  if (num_returns != nullptr) *num_returns = static_cast<int64_t>(ret.size() / 3);
  if (num_misses != nullptr) *num_misses = static_cast<int64_t>(mis.size() / 3);
  return DLIOM_OK;
}

int dliom_node_range_data_from_proto(dliom_ctx* ctx, const uint8_t* bytes, int64_t size, dliom_node_cloud_info* info, dliom_cloud** returns,
                                     dliom_cloud** misses) {
  if (ctx == nullptr || info == nullptr || returns == nullptr || misses == nullptr || size < 0 || (size > 0 && bytes == nullptr))
    return DLIOM_ERR_INVALID_ARGUMENT;
  *returns = *misses = nullptr;
  dliom_node_cloud_info parsed;
  std::vector<float> ret, mis;
  if (!parse_node_range_data(bytes, bytes + size, &parsed, &ret, &mis)) return DLIOM_ERR_INVALID_ARGUMENT;
  int st = dliom_cloud_create(ctx, ret.data(), static_cast<int64_t>(ret.size() / 3), returns);
  if (st == DLIOM_OK) st = dliom_cloud_create(ctx, mis.data(), static_cast<int64_t>(mis.size() / 3), misses);
  if (st != DLIOM_OK) {
    if (*returns != nullptr) dliom_cloud_destroy(*returns);
    *returns = *misses = nullptr;
    return st;
  }
  *info = parsed;
  return DLIOM_OK;
}

}  // extern "C"
