// pcl::ApproximateVoxelGrid<PointXYZ> as PCL 1.8.0 runs it, on the device (dliom.h "the approximate voxel grid"):
// LocalTrajectoryBuilder3D::MatchByNDT filters both of its clouds with it at 0.2 m.  The filter is a sequential loop over a
// table of 512 slots, and its output depends on the stream order -- but only within a slot: the 512 slots are independent
// streams.  The replay:
//   avg_key_kernel    a lane a point: its slot (9 bits) as the sort key; a point the statement refuses raises the flag
//   hipcub radix sort stable, over the 9 key bits: a slot's points come out in stream order
//   avg_head_kernel   a lane a sorted position: does the point start a run (first of its slot, or another voxel than its
//                     predecessor's)?  A run start that is not the first of its slot EVICTS the run before it: its flag goes
//                     to the point's place in STREAM order; the first of a slot marks the slot occupied
//   scan_kept         (compact.hip) the inclusive sum of the evicting flags in stream order: the run a point evicts is the
//                     loop's output number (sum - 1); the last entry is E, the number of evictions
//   avg_rank_kernel   one workgroup: a slot's rank among the occupied ones; the last run of a slot is output E + rank
//   avg_run_kernel    a lane a run start: the three float sums from +0.0 in stream order, the division by (float)count, the
//                     store at the run's output number; the largest squared norm of the centroids
//   read_kept         the call's ONE read-back: E, the largest norm, the number of occupied slots, the refusal flag
//   copy_pad_kernel   (core.hip) the centroids into a cloud of their number
// Every index a kernel forms stays inside its array whatever the points hold: a slot is masked to 9 bits, an output number
// is below the number of runs, which is at most n.  So the kernels may run before the host knows of a refusal.
// What bounds it: the sort and the scan stream 8 and 4 bytes a point; the head and run kernels gather a point by its sorted
// index (12 bytes at a scattered address, a slot's points ascending).  One lane walks one run, so a cloud that lies in a
// single voxel is summed by a single lane: the sums are sequential by definition.
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstring>

#include "device_common.h"

namespace dliom {
namespace {

constexpr int kBlock = 256;
constexpr int kSlots = 512;  // PCL's table
constexpr int kKeyBits = 9;
constexpr int64_t kMaxPoints = int64_t{1} << 30;

struct Voxel {
  int x, y, z;
};
__device__ __forceinline__ bool same_voxel(const Voxel& a, const Voxel& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
// the floor is clamped to what int holds (NaN: 0) before the cast: a cloud with such a point is refused (avg_key_kernel),
// and what the later kernels make of it is discarded, but the cast itself stays defined
__device__ __forceinline__ int index_of(float v) {
  const float f = floorf(v);
  return static_cast<int>(f >= -2147483648.f ? (f < 2147483648.f ? f : 2147483520.f) : (f == f ? -2147483648.f : 0.f));
}
__device__ __forceinline__ Voxel voxel_of(float px, float py, float pz, float inv) {
  return Voxel{index_of(px * inv), index_of(py * inv), index_of(pz * inv)};
}
__device__ __forceinline__ unsigned slot_of(const Voxel& v) {
  return (static_cast<unsigned>(v.x) * 7171u + static_cast<unsigned>(v.y) * 3079u + static_cast<unsigned>(v.z) * 4231u) &
         static_cast<unsigned>(kSlots - 1);
}

// result words behind the occupancy table: the number of occupied slots, the refusal flag
struct AvgWords {
  unsigned occupied[kSlots];
  unsigned num_occupied, refused;
};

__global__ __launch_bounds__(kBlock) void avg_key_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ z, int n, float inv,
                                                         unsigned* __restrict__ keys, int* __restrict__ index, AvgWords* words) {
  const int i = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const float px = x[i], py = y[i], pz = z[i];
  const float f[3] = {floorf(px * inv), floorf(py * inv), floorf(pz * inv)};
  bool ok = isfinite(px) && isfinite(py) && isfinite(pz);
  for (int a = 0; a < 3; ++a) ok = ok && f[a] >= -2147483648.f && f[a] < 2147483648.f;  // the cast to int is defined
  if (!ok) words->refused = 1u;  // the call fails; the point's slot only has to be one
  keys[i] = ok ? slot_of(Voxel{static_cast<int>(f[0]), static_cast<int>(f[1]), static_cast<int>(f[2])}) : 0u;
  index[i] = i;
}

// head[j] = 1 where a run starts; evicts[i] = 1 where point i (stream order) flushes the run before it
__global__ __launch_bounds__(kBlock) void avg_head_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ z, int n, float inv,
                                                          const unsigned* __restrict__ keys, const int* __restrict__ sorted_index,
                                                          int* __restrict__ head, unsigned* __restrict__ evicts, AvgWords* words) {
  const int j = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= n) return;
  const unsigned slot = keys[j] & static_cast<unsigned>(kSlots - 1);
  const int i = sorted_index[j];
  const bool first_of_slot = j == 0 || keys[j - 1] != keys[j];
  bool starts = true;
  if (!first_of_slot) {
    const int before = sorted_index[j - 1];
    starts = !same_voxel(voxel_of(x[i], y[i], z[i], inv), voxel_of(x[before], y[before], z[before], inv));
  }
  head[j] = starts ? 1 : 0;
  evicts[i] = starts && !first_of_slot ? 1u : 0u;
  if (first_of_slot) words->occupied[slot] = 1u;
}

// rank[s] = the occupied slots below s
__global__ __launch_bounds__(kSlots) void avg_rank_kernel(AvgWords* words, unsigned* __restrict__ rank) {
  __shared__ unsigned sums[kSlots];
  const unsigned t = threadIdx.x;
  const unsigned mine = words->occupied[t];
  sums[t] = mine;
  __syncthreads();
  for (unsigned d = 1; d < static_cast<unsigned>(kSlots); d <<= 1) {
    const unsigned add = t >= d ? sums[t - d] : 0u;
    __syncthreads();
    sums[t] += add;
    __syncthreads();
  }
  rank[t] = sums[t] - mine;
  if (t == static_cast<unsigned>(kSlots - 1)) words->num_occupied = sums[t];
}

// The flush of a run: centroid = float sums in stream order / (float)count, at the loop's output number
__global__ __launch_bounds__(kBlock) void avg_run_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ z, int n, float inv,
                                                         const unsigned* __restrict__ keys, const int* __restrict__ sorted_index,
                                                         const int* __restrict__ head, const unsigned* __restrict__ evicts_inclusive,
                                                         const unsigned* __restrict__ rank, float* __restrict__ ox,
                                                         float* __restrict__ oy, float* __restrict__ oz, unsigned* __restrict__ max_sq) {
  const int j = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x;
  unsigned word = 0u;
  if (j < n && head[j] != 0) {
    const unsigned key = keys[j];
    int i = sorted_index[j];
    float px = x[i], py = y[i], pz = z[i];
    const Voxel mine = voxel_of(px, py, pz, inv);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int count = 0, k = j, evictor = -1;
    for (;;) {
      sx += px;
      sy += py;
      sz += pz;
      ++count;
      ++k;
      if (k >= n || keys[k] != key) break;  // the slot's last run: flushed at the end
      i = sorted_index[k];
      px = x[i];
      py = y[i];
      pz = z[i];
      if (!same_voxel(mine, voxel_of(px, py, pz, inv))) {
        evictor = i;
        break;
      }
    }
    const unsigned at = evictor >= 0 ? evicts_inclusive[evictor] - 1u
                                     : evicts_inclusive[n - 1] + rank[key & static_cast<unsigned>(kSlots - 1)];
    if (at < static_cast<unsigned>(n)) {
      const float fc = static_cast<float>(count);
      const float cx = sx / fc, cy = sy / fc, cz = sz / fc;
      ox[at] = cx;
      oy[at] = cy;
      oz[at] = cz;
      word = norm_word(cx, cy, cz);
    }
  }
  note_kept(word, max_sq);
}

}  // namespace

int approximate_voxel_filter_cloud(dliom_ctx* ctx, const dliom_cloud& in, float leaf, dliom_cloud** out) {
  *out = nullptr;
  if (!(leaf > 0.f)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (in.n > kMaxPoints) return DLIOM_ERR_CAPACITY;
  if (in.n == 0) return empty_cloud(ctx, out);
  const int n = static_cast<int>(in.n);
  size_t sort_bytes = 0;
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, static_cast<const unsigned*>(nullptr), static_cast<unsigned*>(nullptr),
                                                   static_cast<const int*>(nullptr), static_cast<int*>(nullptr), n, 0, kKeyBits, ctx->stream));
  const size_t per = align256(4 * static_cast<size_t>(n)), words_bytes = align256(sizeof(AvgWords));
  const size_t rank_bytes = align256(4 * static_cast<size_t>(kSlots));
  CompactScratch s;
  DLIOM_TRY(carve_compact(ctx, n, &s, words_bytes + rank_bytes + 7 * per + align256(sort_bytes), words_bytes));
  char* const e = static_cast<char*>(s.extra);
  AvgWords* const words = reinterpret_cast<AvgWords*>(e);  // zero
  unsigned* const rank = reinterpret_cast<unsigned*>(e + words_bytes);
  char* const a = e + words_bytes + rank_bytes;
  unsigned* const keys_in = reinterpret_cast<unsigned*>(a);
  unsigned* const keys = reinterpret_cast<unsigned*>(a + per);
  int* const index_in = reinterpret_cast<int*>(a + 2 * per);
  int* const sorted_index = reinterpret_cast<int*>(a + 3 * per);
  float* const ox = reinterpret_cast<float*>(a + 4 * per);
  float* const oy = reinterpret_cast<float*>(a + 5 * per);
  float* const oz = reinterpret_cast<float*>(a + 6 * per);
  void* const sort_tmp = a + 7 * per;
  const float inv = 1.0f / leaf;
  const dim3 grid(blocks_of(n, kBlock)), block(kBlock);
  hipLaunchKernelGGL(avg_key_kernel, grid, block, 0, ctx->stream, in.d_x, in.d_y, in.d_z, n, inv, keys_in, index_in, words);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, keys_in, keys, index_in, sorted_index, n, 0, kKeyBits, ctx->stream));
  // s.index: the run starts, by sorted position; s.keep: the evicting points, by stream position
  hipLaunchKernelGGL(avg_head_kernel, grid, block, 0, ctx->stream, in.d_x, in.d_y, in.d_z, n, inv, keys, sorted_index, s.index, s.keep, words);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_TRY(scan_kept(ctx, n, s));
  hipLaunchKernelGGL(avg_rank_kernel, dim3(1), dim3(kSlots), 0, ctx->stream, words, rank);
  DLIOM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(avg_run_kernel, grid, block, 0, ctx->stream, in.d_x, in.d_y, in.d_z, n, inv, keys, sorted_index, s.index, s.inclusive,
                     rank, ox, oy, oz, s.max_sq);
  DLIOM_HIP_TRY(hipGetLastError());
  const GatherJob more{&words->num_occupied, 2};
  int64_t evictions = 0;
  float max_sq = 0.f;
  unsigned tail[2] = {0u, 0u};
  DLIOM_TRY(read_kept(ctx, n, s, &more, &evictions, &max_sq, tail));
  if (tail[1] != 0u) return DLIOM_ERR_INVALID_ARGUMENT;
  const int64_t runs = evictions + static_cast<int64_t>(tail[0]);
  if (runs <= 0 || runs > n) return DLIOM_ERR_INTERNAL;
  float *x, *y, *z;
  DLIOM_TRY(alloc_device_cloud(ctx, runs, out, &x, &y, &z));
  const int st = finish_device_cloud_from(ctx, *out, std::sqrt(max_sq), ox, oy, oz);  // sqrt is monotone: the max of the norms
  if (st != DLIOM_OK) {
    dliom_cloud_destroy(*out);
    *out = nullptr;
  }
  return st;
}

}  // namespace dliom

extern "C" {

int dliom_cloud_approximate_voxel_filter(dliom_ctx* ctx, const dliom_cloud* in, float leaf, dliom_cloud** out) {
  if (out != nullptr) *out = nullptr;
  if (ctx == nullptr || in == nullptr || out == nullptr || in->ctx != ctx) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  return dliom::approximate_voxel_filter_cloud(ctx, *in, leaf, out);
}

}  // extern "C"
