// FastCorrelativeScanMatcher3D (loop-closure branch and bound) on the device.
//
//   mapping/internal/3d/scan_matching/precomputation_grid_3d.cc:49-82   uint8 max-pool pyramid
//   mapping/internal/3d/scan_matching/fast_correlative_scan_matcher_3d.cc
//       :57-77   PrecomputationGridStack3D        -> convert_level0_kernel, precompute_level_kernel
//       :264-304 DiscretizeScan                   -> discretize_kernel (cells per discrete scan)
//       :394-417 ScoreCandidates                  -> score_candidates_kernel (exact integer sums)
//       :439-492 BranchAndBound                   -> host recursion (same order, same std::sort),
//                                                    scores served from a cache that the device
//                                                    fills in batches
//   mapping/internal/3d/scan_matching/rotational_scan_matcher.cc:125-194 histogram matching (host)
//   mapping/internal/3d/scan_matching/low_resolution_matcher.cc:23-36   -> the exact sequential
//                                                    float sum kernels of sequential_sums.hip
//
// Exactness: a candidate's score is ToProbability(sum / float(N)) of an INTEGER sum, so any
// summation order on the device gives the reference's float; the traversal (which candidates are
// expanded, in which order equal scores are visited) is replayed on the host with the reference's
// own comparisons and std::sort calls.  The pyramid levels are dense uint8 boxes over the bounding
// box of the submap's leaves (a max-pool is order independent); cells outside read 0 like
// HybridGridBase<uint8>::value() of an unset cell.
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <unordered_map>
#include <vector>

#include "device_common.h"
#include "host_math.h"
#include "internal.h"
#include "probability_values.h"
#include "rotational.h"

namespace dliom {

struct LevelView {
  const uint8_t* data;
  int lo[3];  // cell index of element (0,0,0)
  int n[3];   // cells per axis (0: empty level)
};

__device__ __forceinline__ unsigned level_value(const LevelView& l, int x, int y, int z) {
  const unsigned ux = static_cast<unsigned>(x - l.lo[0]), uy = static_cast<unsigned>(y - l.lo[1]),
                 uz = static_cast<unsigned>(z - l.lo[2]);
  if (ux >= static_cast<unsigned>(l.n[0]) || uy >= static_cast<unsigned>(l.n[1]) || uz >= static_cast<unsigned>(l.n[2]))
    return 0u;
  return l.data[(static_cast<size_t>(uz) * l.n[1] + uy) * l.n[0] + ux];
}

// Bounding box of the allocated leaves (leaf coordinates = voxel index >> 3): mm[0..2] min, [3..5] max.
__global__ void leaf_bbox_kernel(const int32_t* __restrict__ slot_coord, unsigned count, int* __restrict__ mm) {
  const unsigned s = blockIdx.x * blockDim.x + threadIdx.x + 1;  // slot 0 is the null leaf
  if (s >= count) return;
  for (int a = 0; a < 3; ++a) {
    const int c = slot_coord[3 * static_cast<size_t>(s) + a];
    atomicMin(&mm[a], c);
    atomicMax(&mm[3 + a], c);
  }
}

// ConvertToPrecomputationGrid: one workgroup per leaf, cell = lut8[value & 0x7fff].
__global__ void convert_level0_kernel(const int32_t* __restrict__ slot_coord, const uint16_t* __restrict__ pool,
                                      const uint8_t* __restrict__ lut8, uint8_t* __restrict__ out, int lox, int loy,
                                      int loz, int nx, int ny) {
  const size_t s = static_cast<size_t>(blockIdx.x) + 1;
  const int bx = slot_coord[3 * s] * 8 - lox, by = slot_coord[3 * s + 1] * 8 - loy, bz = slot_coord[3 * s + 2] * 8 - loz;
  for (int c = threadIdx.x; c < 512; c += blockDim.x) {
    const unsigned v = pool[s * 512 + c] & 0x7FFFu;
    out[(static_cast<size_t>(bz + (c >> 6)) * ny + (by + ((c >> 3) & 7))) * nx + (bx + (c & 7))] = lut8[v];
  }
}

// PrecomputeGrid as a gather: dst(t) = max over the source cells c and octants o with
// (c - shift o) [>> 1] == t  (8 sources at full resolution, 64 when the resolution halves).
__global__ void precompute_level_kernel(LevelView src, uint8_t* __restrict__ dst, int dlox, int dloy, int dloz, int dnx,
                                        int dny, int dnz, int shift, int half) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t total = static_cast<size_t>(dnx) * dny * dnz;
  if (i >= total) return;
  const int tx = static_cast<int>(i % dnx) + dlox, ty = static_cast<int>((i / dnx) % dny) + dloy,
            tz = static_cast<int>(i / (static_cast<size_t>(dnx) * dny)) + dloz;
  unsigned m = 0;
  const int sub = half ? 2 : 1;
  for (int oz = 0; oz < 2; ++oz)
    for (int sz = 0; sz < sub; ++sz)
      for (int oy = 0; oy < 2; ++oy)
        for (int sy = 0; sy < sub; ++sy)
          for (int ox = 0; ox < 2; ++ox)
            for (int sx = 0; sx < sub; ++sx) {
              const int cx = (half ? 2 * tx + sx : tx) + shift * ox, cy = (half ? 2 * ty + sy : ty) + shift * oy,
                        cz = (half ? 2 * tz + sz : tz) + shift * oz;
              m = max(m, level_value(src, cx, cy, cz));
            }
  dst[i] = static_cast<uint8_t>(m);
}

// DiscretizeScan: cell index of pose_s * p for every discrete scan s and point p.
__device__ __forceinline__ void discretize_point(const float* pose7, float px, float py, float pz, float resolution, int* cx,
                                                 int* cy, int* cz) {
  const Quat4 q{pose7[3], pose7[4], pose7[5], pose7[6]};
  float rx, ry, rz;
  rotate_point(q, px, py, pz, rx, ry, rz);
  *cx = cell_of(rx + pose7[0], resolution);
  *cy = cell_of(ry + pose7[1], resolution);
  *cz = cell_of(rz + pose7[2], resolution);
}
__global__ void discretize_kernel(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                  int n, const float* __restrict__ poses7, float resolution, int* __restrict__ cx,
                                  int* __restrict__ cy, int* __restrict__ cz) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = blockIdx.y;
  const size_t o = static_cast<size_t>(s) * n + i;
  discretize_point(poses7 + 7 * s, px[i], py[i], pz[i], resolution, &cx[o], &cy[o], &cz[o]);
}
// The discrete scans of a whole batch (dliom_fast_csm_match_batch): blockIdx.y = scan across every query of the batch.
struct DiscreteScanArg {
  const float* pts;  // the query's high-resolution cloud, packed xyz
  int *cx, *cy, *cz; // this scan's row of the query's [scan][point] cells
  int n;
  float resolution;
  float pose[7];
};
__global__ __launch_bounds__(256) void discretize_batch_kernel(const DiscreteScanArg* __restrict__ scans) {
  const DiscreteScanArg& a = scans[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  discretize_point(a.pose, a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2], a.resolution, &a.cx[i], &a.cy[i], &a.cz[i]);
}

struct ScoreArgs {
  LevelView level;
  const int *cx, *cy, *cz;  // [scan][point] full-resolution cells
  int n;                    // points per scan
  int e;                    // reduction exponent max(0, depth - full_resolution_depth + 1)
  int start[3];             // search_window_start (negative window sizes)
};

// ScoreCandidates: blockIdx.x = candidate (scan, full-resolution offset), blockIdx.y = chunk of
// kScoreChunk points; lanes over points, block reduction, one atomicAdd per (candidate, chunk).
constexpr int kScoreChunk = 2048;
__global__ __launch_bounds__(256) void score_candidates_kernel(ScoreArgs a, const int4* __restrict__ candidates,
                                                               int num_candidates, int* __restrict__ sums) {
  __shared__ unsigned wave_sums[4];
  const int c = blockIdx.x;
  const int4 cand = candidates[c];
  const int ox = cand.y >> a.e, oy = cand.z >> a.e, oz = cand.w >> a.e;
  const int lsx = a.start[0] >> a.e, lsy = a.start[1] >> a.e, lsz = a.start[2] >> a.e;
  const size_t base = static_cast<size_t>(cand.x) * a.n;
  const int p_begin = blockIdx.y * kScoreChunk, p_end = min(a.n, p_begin + kScoreChunk);
  unsigned sum = 0;
  for (int p = p_begin + threadIdx.x; p < p_end; p += 256) {
    int x = a.cx[base + p], y = a.cy[base + p], z = a.cz[base + p];
    if (a.e > 0) {  // low-resolution cells (:285-301)
      x = ((x + a.start[0]) >> a.e) - lsx;
      y = ((y + a.start[1]) >> a.e) - lsy;
      z = ((z + a.start[2]) >> a.e) - lsz;
    }
    sum += level_value(a.level, x + ox, y + oy, z + oz);
  }
  sum = wave_sum_lane63(sum);
  if ((threadIdx.x & 63) == 63) wave_sums[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&sums[c], static_cast<int>(wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3]));
}


// ---- device frontier -----------------------------------------------------------------------------
// BranchAndBound (:439-492) asks for the scores of the children of every node whose score beats the best leaf found
// so far.  Served one sibling group per launch that is ~110 launches + synchronisations for a whole-submap window
// on a filtered scan (150 points): 3 ms, all of it latency.  Instead ONE chain of launches, no host in between:
//   1. the lowest-resolution candidates (host list) are scored;
//   2. one workgroup walks the branch the recursion walks first -- best candidate, best child, ... down to a leaf --
//      whose score theta is (up to ties and the low-resolution check) the bound the recursion prunes with from its
//      first leaf on;
//   3. level by level, the children of every node with score >= max(theta, min_score) are scored and appended to
//      that level's list: a superset of everything the recursion can ask for once it holds a leaf of score theta,
//      and (>=, upper bounds) of the branch it walks before;
//   4. all lists are packed into pinned host memory; one synchronisation.
// The host then replays the reference's recursion -- same comparisons, same std::sort calls -- out of a hash table;
// anything missing (a first leaf refused by the low-resolution matcher, a list that hit its capacity) is fetched
// on demand as before.  Exactness is untouched: scores are functions of exact integer sums.
constexpr int kMaxLevels = 16;
constexpr int kCountWords = 64;  // per search: [kMaxLevels] records per list, [kMaxLevels] overflow flag, [kMaxLevels + 1] theta
struct FrontierRec {
  int scan, ox, oy, oz, sum;
};
// One search of a chain.  The chain serves any number of searches (the single calls: one); their arguments live in a
// device array, each with its own level views, window, depth, record pool, counts and output region.
struct FrontierArgs {
  LevelView level[kMaxLevels];
  const int *cx, *cy, *cz;  // [scan][point] full-resolution cells
  int n;                    // points per scan
  int max_depth, full_resolution_depth;
  int linear_xy, linear_z;
  FrontierRec* pool;        // (max_depth + 1) lists of `cap` records, list d at pool + d * cap
  int* counts;              // kCountWords
  int cap;
  float min_score;
  int top_begin, top_count; // this search's lowest-resolution candidates in the chain's flat list
  int* out;                 // page-locked: [counts | overflow | theta | records of list max_depth, ..., 0]
  int out_records;
};

__device__ __forceinline__ float frontier_probability(int sum, int n) {  // ScoreCandidates' float (:407-411)
  return kMinProbability + (static_cast<float>(sum) / static_cast<float>(n)) * ((kMaxProbability - kMinProbability) / 255.f);
}

// Integer sum of one candidate at `depth`, by one wavefront (every lane returns it).
__device__ __forceinline__ int frontier_wave_sum(const FrontierArgs& a, int depth, int scan, int ox, int oy, int oz, int lane) {
  const int e = max(0, depth - a.full_resolution_depth + 1);
  const int sx = -a.linear_xy, sz = -a.linear_z;
  const int lsx = sx >> e, lsz = sz >> e;
  const LevelView& lv = a.level[depth];
  const size_t base = static_cast<size_t>(scan) * a.n;
  const int cox = ox >> e, coy = oy >> e, coz = oz >> e;
  unsigned sum = 0;
  for (int p = lane; p < a.n; p += 64) {
    int x = a.cx[base + p], y = a.cy[base + p], z = a.cz[base + p];
    if (e > 0) {  // low-resolution cells (:285-301)
      x = ((x + sx) >> e) - lsx;
      y = ((y + sx) >> e) - lsx;
      z = ((z + sz) >> e) - lsz;
    }
    sum += level_value(lv, x + cox, y + coy, z + coz);
  }
  return __builtin_amdgcn_readlane(static_cast<int>(wave_sum_lane63(sum)), 63);
}

// 1. sums of the flat list of every search's lowest-resolution candidates, one wavefront per candidate; each record
//    goes to list max_depth of its search
__global__ __launch_bounds__(256) void frontier_top_kernel(const FrontierArgs* __restrict__ args, int num_searches,
                                                           const FrontierRec* __restrict__ flat, int total) {
  const int w = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (w >= total) return;
  int lo = 0, hi = num_searches - 1;  // the search whose range holds w
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (args[mid].top_begin <= w) lo = mid; else hi = mid - 1;
  }
  const FrontierArgs& a = args[lo];
  FrontierRec r = flat[w];
  r.sum = frontier_wave_sum(a, a.max_depth, r.scan, r.ox, r.oy, r.oz, lane);
  if (lane == 0) a.pool[static_cast<size_t>(a.max_depth) * a.cap + (w - a.top_begin)] = r;
}

// 2. the branch the recursion walks first; writes theta.  One workgroup per search.
__global__ __launch_bounds__(512) void frontier_greedy_kernel(const FrontierArgs* __restrict__ args) {
  __shared__ unsigned long long best_key[8];
  __shared__ int child_sum[8];
  __shared__ int cur[4];
  const FrontierArgs& a = args[blockIdx.x];
  const int top_count = a.top_count;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const FrontierRec* top = a.pool + static_cast<size_t>(a.max_depth) * a.cap;
  unsigned long long key = 0ull;
  for (int i = threadIdx.x; i < top_count; i += blockDim.x)
    key = max(key, (static_cast<unsigned long long>(static_cast<unsigned>(top[i].sum)) << 32) | static_cast<unsigned>(0x7FFFFFFF - i));
  for (int m = 32; m >= 1; m >>= 1) key = max(key, __shfl_xor(key, m));
  if (lane == 0) best_key[wave] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long k = 0ull;
    for (int w = 0; w < 8; ++w) k = max(k, best_key[w]);
    const int i = 0x7FFFFFFF - static_cast<int>(k & 0xFFFFFFFFull);
    cur[0] = top[i].scan;
    cur[1] = top[i].ox;
    cur[2] = top[i].oy;
    cur[3] = top[i].oz;
    child_sum[0] = static_cast<int>(k >> 32);
  }
  __syncthreads();
  int sum = child_sum[0];
  __syncthreads();
  for (int depth = a.max_depth; depth >= 1; --depth) {
    const int hw = 1 << (depth - 1);
    const int scan = cur[0], ox = cur[1] + ((wave & 1) ? hw : 0), oy = cur[2] + ((wave & 2) ? hw : 0), oz = cur[3] + ((wave & 4) ? hw : 0);
    const bool valid = ox <= a.linear_xy && oy <= a.linear_xy && oz <= a.linear_z;  // children_of (:468-484)
    const int s = valid ? frontier_wave_sum(a, depth - 1, scan, ox, oy, oz, lane) : -1;
    if (lane == 0) child_sum[wave] = s;
    __syncthreads();
    int bw = 0;
    for (int w = 1; w < 8; ++w)
      if (child_sum[w] > child_sum[bw]) bw = w;
    sum = child_sum[bw];
    __syncthreads();
    if (threadIdx.x == 0) {
      cur[1] += (bw & 1) ? hw : 0;
      cur[2] += (bw & 2) ? hw : 0;
      cur[3] += (bw & 4) ? hw : 0;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float theta = fmaxf(frontier_probability(sum, a.n), a.min_score);
    a.counts[kMaxLevels + 1] = __float_as_int(theta);
  }
}

// 3. list `depth` -> list depth - 1: the children of every node with score >= theta, one wavefront per child.
//    blockIdx.y = search; a search whose pyramid is shallower than `depth` has nothing to do in this launch.
__global__ __launch_bounds__(256) void frontier_level_kernel(const FrontierArgs* __restrict__ args, int depth) {
  const FrontierArgs& a = args[blockIdx.y];
  if (depth > a.max_depth) return;
  const int lane = threadIdx.x & 63;
  const int waves = (gridDim.x * blockDim.x) >> 6;
  const int parents = min(a.counts[depth], a.cap);
  const float theta = __int_as_float(a.counts[kMaxLevels + 1]);
  const FrontierRec* src = a.pool + static_cast<size_t>(depth) * a.cap;
  FrontierRec* dst = a.pool + static_cast<size_t>(depth - 1) * a.cap;
  const int hw = 1 << (depth - 1);
  for (int item = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; item < 8 * parents; item += waves) {
    const FrontierRec pr = src[item >> 3];
    if (!(frontier_probability(pr.sum, a.n) >= theta)) continue;
    const int c = item & 7;
    const int ox = pr.ox + ((c & 1) ? hw : 0), oy = pr.oy + ((c & 2) ? hw : 0), oz = pr.oz + ((c & 4) ? hw : 0);
    if (ox > a.linear_xy || oy > a.linear_xy || oz > a.linear_z) continue;
    const int sum = frontier_wave_sum(a, depth - 1, pr.scan, ox, oy, oz, lane);
    if (lane == 0) {
      const int at = atomicAdd(&a.counts[depth - 1], 1);
      if (at < a.cap)
        dst[at] = FrontierRec{pr.scan, ox, oy, oz, sum};
      else
        a.counts[kMaxLevels] = 1;  // overflow: the host fetches what is missing on demand
    }
  }
}

// 4. [counts | overflow | theta | records of list max_depth, ..., 0] -> the search's page-locked region (blockIdx.y)
__global__ __launch_bounds__(256) void frontier_pack_kernel(const FrontierArgs* __restrict__ args) {
  const FrontierArgs& a = args[blockIdx.y];
  int* out = a.out;
  const int out_records = a.out_records;
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;
  if (tid < kMaxLevels + 2) out[tid] = a.counts[tid];
  int first = 0;
  for (int depth = a.max_depth; depth >= 0; --depth) {
    const int cnt = min(a.counts[depth], a.cap);
    const int* src = reinterpret_cast<const int*>(a.pool + static_cast<size_t>(depth) * a.cap);
    for (int i = tid; i < 5 * cnt; i += nthreads)
      if (first + i / 5 < out_records) out[kMaxLevels + 2 + 5 * first + i] = src[i];
    first += cnt;
  }
}

// ---- host side ---------------------------------------------------------------------------------
// rotate_histogram / match_histograms live in rotational_histogram.cc (host-only, CPU-testable).
using Histogram = std::vector<float>;

static QF quat_inverse(const QF& q) {  // Eigen QuaternionBase::inverse()
  const float n2 = (q.x * q.x + q.z * q.z) + (q.y * q.y + q.w * q.w);
  if (n2 > 0.f) return QF{q.w / n2, -q.x / n2, -q.y / n2, -q.z / n2};
  return QF{0.f, 0.f, 0.f, 0.f};
}
static float get_yaw(const QF& q) {  // transform/transform.h:41-46
  const F3 d = qrot(q, F3{1.f, 0.f, 0.f});
  return std::atan2(d.y, d.x);
}
static PoseF pose_mul_f(const PoseF& a, const PoseF& b) {  // rigid_transform.h:206-212
  return PoseF{add3(qrot(a.q, b.t), a.t), qnormalized(qmul(a.q, b.q))};
}
static PoseF pose_inverse_f(const PoseF& a) {  // rigid_transform.h:167-171
  const QF r{a.q.w, -a.q.x, -a.q.y, -a.q.z};
  const F3 t = qrot(r, a.t);
  return PoseF{F3{-t.x, -t.y, -t.z}, r};
}

}  // namespace dliom

using namespace dliom;

struct dliom_fast_csm {
  dliom_ctx* ctx = nullptr;
  dliom_fast_csm_options options;
  float resolution = 0.f;
  int width_in_voxels = 0;
  const dliom_grid* lo_grid = nullptr;
  Histogram submap_histogram;
  struct Level {
    uint8_t* d = nullptr;
    int lo[3] = {0, 0, 0};
    int n[3] = {0, 0, 0};
    size_t cells() const { return static_cast<size_t>(n[0]) * n[1] * n[2]; }
    LevelView view() const { return LevelView{d, {lo[0], lo[1], lo[2]}, {n[0], n[1], n[2]}}; }
  };
  std::vector<Level> levels;
  int max_depth() const { return static_cast<int>(levels.size()) - 1; }
  ~dliom_fast_csm() {
    for (Level& l : levels)
      if (l.d != nullptr) (void)hipFree(l.d);
  }
};

namespace {

struct Candidate {
  int scan_index;
  int offset[3];
  float score = -std::numeric_limits<float>::infinity();
  float low_resolution_score = 0.f;
  bool operator<(const Candidate& o) const { return score < o.score; }
  bool operator>(const Candidate& o) const { return score > o.score; }
};

struct Search {
  const dliom_fast_csm* m;
  dliom_ctx* ctx;  // the CALLER's context: scratch, stream, pinned block (the matcher itself is read-only)
  int linear_xy, linear_z;
  double angular_window;
  // per match
  std::vector<PoseF> scan_poses;
  std::vector<float> rotational_scores;
  int n_hi = 0;
  int64_t n_lo = 0;  // the batch: points of the low-resolution cloud (lo_cloud is made per chunk)
  int *d_cx = nullptr, *d_cy = nullptr, *d_cz = nullptr;
  const dliom_cloud* lo_cloud = nullptr;
  float min_low_resolution_score_f = 0.f;
  long long scored = 0;
  long long launches = 0;
  const std::vector<Candidate>* top = nullptr;  // the sorted lowest-resolution candidates
  float initial_min_score = 0.f;
  float frontier_threshold = std::numeric_limits<float>::infinity();  // last wavefront prefetch ran with this
  long long syncs = 0;         // stream synchronisations of this search's on-demand fetches
  long long cache_misses = 0;  // scores fetched on demand
  // low-resolution sums of leaves a batch scored ahead (key(0, scan, offset) -> sequential float sum); empty otherwise
  std::unordered_map<uint64_t, float> low_sums;
  // score cache: (depth, scan, offset) -> integer sum.  Open addressing, linear probing (a match looks up and inserts
  // ~1e4 keys: std::unordered_map's node allocations were a third of the host time of a whole-submap match)
  struct ScoreCache {
    static constexpr uint64_t kEmpty = ~0ull;
    std::vector<uint64_t> keys;
    std::vector<int> vals;
    size_t used = 0;
    ScoreCache() { rehash(1u << 12); }
    static size_t mix(uint64_t k) {
      k ^= k >> 33;
      k *= 0xff51afd7ed558ccdull;
      k ^= k >> 33;
      return static_cast<size_t>(k);
    }
    void rehash(size_t cap) {
      std::vector<uint64_t> ok;
      std::vector<int> ov;
      ok.swap(keys);
      ov.swap(vals);
      keys.assign(cap, kEmpty);
      vals.assign(cap, 0);
      used = 0;
      for (size_t i = 0; i < ok.size(); ++i)
        if (ok[i] != kEmpty) put(ok[i], ov[i]);
    }
    const int* get(uint64_t k) const {
      const size_t mask = keys.size() - 1;
      for (size_t i = mix(k) & mask;; i = (i + 1) & mask) {
        if (keys[i] == k) return &vals[i];
        if (keys[i] == kEmpty) return nullptr;
      }
    }
    bool has(uint64_t k) const { return get(k) != nullptr; }
    void put(uint64_t k, int v) {
      if (2 * (used + 1) > keys.size()) rehash(2 * keys.size());
      const size_t mask = keys.size() - 1;
      for (size_t i = mix(k) & mask;; i = (i + 1) & mask) {
        if (keys[i] == k) {
          vals[i] = v;
          return;
        }
        if (keys[i] == kEmpty) {
          keys[i] = k;
          vals[i] = v;
          ++used;
          return;
        }
      }
    }
  } cache;
  static uint64_t key(int depth, int scan, const int* o) {
    // offsets fit 14 bits + sign for any window the 8-bit grid extent allows; scans < 2^16
    return (static_cast<uint64_t>(depth & 0xF) << 60) | (static_cast<uint64_t>(scan & 0xFFFF) << 44) |
           (static_cast<uint64_t>((o[0] + 8192) & 0x3FFF) << 28) | (static_cast<uint64_t>((o[1] + 8192) & 0x3FFF) << 14) |
           static_cast<uint64_t>((o[2] + 8192) & 0x3FFF);
  }
  static uint64_t key(int depth, const Candidate& c) { return key(depth, c.scan_index, c.offset); }
};

// a candidate <-> its record in the device frontier's lists; a float pose -> t, q (w, x, y, z) as floats or doubles
inline Candidate to_candidate(const FrontierRec& r) { return Candidate{r.scan, {r.ox, r.oy, r.oz}}; }
inline FrontierRec to_rec(const Candidate& c) { return FrontierRec{c.scan_index, c.offset[0], c.offset[1], c.offset[2], 0}; }
template <class T>
inline void pose7(const PoseF& p, T* out) {
  const T v[7] = {p.t.x, p.t.y, p.t.z, p.q.w, p.q.x, p.q.y, p.q.z};
  std::memcpy(out, v, sizeof(v));
}

// Integer sums of `list` at `depth` (device), in list order.
int device_sums(Search& s, int depth, const std::vector<Candidate>& list, std::vector<int>* sums) {
  const dliom_fast_csm* m = s.m;
  dliom_ctx* ctx = s.ctx;
  const size_t k = list.size();
  sums->assign(k, 0);
  if (k == 0) return DLIOM_OK;
  const size_t cbytes = align256(k * 16);
  DLIOM_TRY(ctx->cand.reserve(cbytes + k * 4));
  // candidate list and sums travel through the pinned block when they fit (no staging copies)
  const bool pinned = cbytes + k * 4 <= kPinFastCsmScores.bytes;
  std::vector<int> pageable;
  int* host = pinned_at<int>(ctx, kPinFastCsmScores);
  if (!pinned) {
    pageable.resize(4 * k + k);
    host = pageable.data();
  }
  for (size_t i = 0; i < k; ++i) {
    host[4 * i] = list[i].scan_index;
    host[4 * i + 1] = list[i].offset[0];
    host[4 * i + 2] = list[i].offset[1];
    host[4 * i + 3] = list[i].offset[2];
  }
  int4* d_cand = ctx->cand.as<int4>();
  int* d_sums = reinterpret_cast<int*>(static_cast<char*>(ctx->cand.p) + cbytes);
  DLIOM_HIP_TRY(hipMemcpyAsync(d_cand, host, k * 16, hipMemcpyHostToDevice, ctx->stream));
  DLIOM_HIP_TRY(hipMemsetAsync(d_sums, 0, k * 4, ctx->stream));
  ScoreArgs a;
  a.level = m->levels[depth].view();
  a.cx = s.d_cx;
  a.cy = s.d_cy;
  a.cz = s.d_cz;
  a.n = s.n_hi;
  a.e = std::max(0, depth - m->options.full_resolution_depth + 1);
  a.start[0] = -s.linear_xy;
  a.start[1] = -s.linear_xy;
  a.start[2] = -s.linear_z;
  const unsigned chunks = static_cast<unsigned>((s.n_hi + kScoreChunk - 1) / kScoreChunk);
  hipLaunchKernelGGL(score_candidates_kernel, dim3(static_cast<unsigned>(k), chunks), dim3(256), 0, ctx->stream, a, d_cand,
                     static_cast<int>(k), d_sums);
  DLIOM_HIP_TRY(hipGetLastError());
  int* host_sums = host + 4 * k;
  DLIOM_HIP_TRY(hipMemcpyAsync(host_sums, d_sums, k * 4, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  ++s.syncs;
  s.cache_misses += static_cast<long long>(k);
  std::memcpy(sums->data(), host_sums, k * 4);
  s.scored += static_cast<long long>(k);
  ++s.launches;
  return DLIOM_OK;
}

inline float to_probability(float value) {  // precomputation_grid_3d.h:31-34
  return kMinProbability + value * ((kMaxProbability - kMinProbability) / 255.f);
}

// Appends to `missing` those of `list` whose sum at `depth` the cache lacks.
void append_missing(const Search& s, int depth, const std::vector<Candidate>& list, std::vector<Candidate>* missing) {
  for (const Candidate& c : list)
    if (!s.cache.has(Search::key(depth, c))) missing->push_back(c);
}
// The sums of `missing` at `depth`: from the device into the cache.
int fetch_sums(Search& s, int depth, const std::vector<Candidate>& missing) {
  if (missing.empty()) return DLIOM_OK;
  std::vector<int> sums;
  DLIOM_TRY(device_sums(s, depth, missing, &sums));
  for (size_t i = 0; i < missing.size(); ++i) s.cache.put(Search::key(depth, missing[i]), sums[i]);
  return DLIOM_OK;
}
// ScoreCandidates' float (:407-411) of a candidate whose sum is in the cache.
float cached_score(const Search& s, int depth, const Candidate& c) {
  return to_probability(*s.cache.get(Search::key(depth, c)) / static_cast<float>(s.n_hi));
}

// ScoreCandidates (:394-417) with the sums served from the cache (filled here when missing).
int score_candidates(Search& s, int depth, std::vector<Candidate>* candidates) {
  std::vector<Candidate> missing;
  append_missing(s, depth, *candidates, &missing);
  DLIOM_TRY(fetch_sums(s, depth, missing));
  for (Candidate& c : *candidates) c.score = cached_score(s, depth, c);
  std::sort(candidates->begin(), candidates->end(), std::greater<Candidate>());
  return DLIOM_OK;
}

void children_of(const Search& s, const Candidate& c, int candidate_depth, std::vector<Candidate>* out) {  // :468-484
  const int half_width = 1 << (candidate_depth - 1);
  for (int z : {0, half_width}) {
    if (c.offset[2] + z > s.linear_z) break;
    for (int y : {0, half_width}) {
      if (c.offset[1] + y > s.linear_xy) break;
      for (int x : {0, half_width}) {
        if (c.offset[0] + x > s.linear_xy) break;
        Candidate h;
        h.scan_index = c.scan_index;
        h.offset[0] = c.offset[0] + x;
        h.offset[1] = c.offset[1] + y;
        h.offset[2] = c.offset[2] + z;
        out->push_back(h);
      }
    }
  }
}

// Batch prefetch: the children of every candidate of `siblings` from position `first` on whose
// score still beats `min_score` -- the group the recursion is about to walk through.
int prefetch_children(Search& s, const std::vector<Candidate>& siblings, size_t first, int candidate_depth,
                      float min_score) {
  std::vector<Candidate> batch;
  for (size_t i = first; i < siblings.size() && batch.size() < 4096; ++i) {
    if (siblings[i].score <= min_score) break;
    std::vector<Candidate> ch;
    children_of(s, siblings[i], candidate_depth, &ch);
    append_missing(s, candidate_depth - 1, ch, &batch);
  }
  return fetch_sums(s, candidate_depth - 1, batch);
}

// Wavefront prefetch: once a first match has raised the bound, every node the recursion can still
// expand has a score above `threshold` -- score the children of ALL such nodes level by level
// (one launch per level) instead of one launch per sibling group.
int prefetch_frontier(Search& s, float threshold) {
  const int top_depth = s.m->max_depth();
  std::vector<Candidate> frontier;
  for (const Candidate& c : *s.top)
    if (c.score > threshold) frontier.push_back(c);
  for (int depth = top_depth; depth >= 1 && !frontier.empty(); --depth) {
    std::vector<Candidate> children;
    for (const Candidate& c : frontier) children_of(s, c, depth, &children);
    if (children.size() > (1u << 18)) break;  // a flat score landscape: stay with on-demand batches
    std::vector<Candidate> missing;
    append_missing(s, depth - 1, children, &missing);
    DLIOM_TRY(fetch_sums(s, depth - 1, missing));
    frontier.clear();
    for (Candidate& c : children) {
      c.score = cached_score(s, depth - 1, c);
      if (c.score > threshold) frontier.push_back(c);
    }
  }
  s.frontier_threshold = threshold;
  return DLIOM_OK;
}

// The device frontier (kernels above): one chain of launches that puts the lowest-resolution candidates and
// everything the recursion can reach below them into a page-locked region per search.  `h` (page-locked) and `d`
// (device) hold the same upload: the array of num_searches FrontierArgs, at frontier_counts_at() num_searches x
// kCountWords counts, then the flat list of `total` lowest-resolution records.  Enqueued only: the caller synchronises.
constexpr size_t frontier_counts_at(int num_searches) {
  return align256(num_searches * sizeof(FrontierArgs));
}
constexpr size_t frontier_flat_at(int num_searches) { return frontier_counts_at(num_searches) + num_searches * kCountWords * 4; }
constexpr size_t frontier_upload_bytes(int num_searches, size_t total) {
  return frontier_flat_at(num_searches) + total * sizeof(FrontierRec);
}
int enqueue_frontier_chain(dliom_ctx* ctx, int num_searches, int total, int deepest, const char* d) {
  const FrontierArgs* args = reinterpret_cast<const FrontierArgs*>(d);
  const FrontierRec* flat = reinterpret_cast<const FrontierRec*>(d + frontier_flat_at(num_searches));
  hipLaunchKernelGGL(frontier_top_kernel, dim3(static_cast<unsigned>((total + 3) / 4)), dim3(256), 0, ctx->stream, args,
                     num_searches, flat, total);
  hipLaunchKernelGGL(frontier_greedy_kernel, dim3(static_cast<unsigned>(num_searches)), dim3(512), 0, ctx->stream, args);
  // 256 workgroups over the whole chain (the single search's grid), at least two per search
  const unsigned per_search = static_cast<unsigned>(std::max(2, 256 / num_searches));
  for (int depth = deepest; depth >= 1; --depth)
    hipLaunchKernelGGL(frontier_level_kernel, dim3(per_search, static_cast<unsigned>(num_searches)), dim3(256), 0, ctx->stream,
                       args, depth);
  hipLaunchKernelGGL(frontier_pack_kernel, dim3(static_cast<unsigned>(std::max(1, 64 / num_searches)), static_cast<unsigned>(num_searches)),
                     dim3(256), 0, ctx->stream, args);
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

// The search's FrontierArgs, except where its pool, counts, upload range and output live.
FrontierArgs frontier_args(const Search& s, float min_score) {
  const dliom_fast_csm* m = s.m;
  FrontierArgs a;
  const int max_depth = m->max_depth();
  for (int d = 0; d < kMaxLevels; ++d) a.level[d] = d <= max_depth ? m->levels[d].view() : LevelView{nullptr, {0, 0, 0}, {0, 0, 0}};
  a.cx = s.d_cx;
  a.cy = s.d_cy;
  a.cz = s.d_cz;
  a.n = s.n_hi;
  a.max_depth = max_depth;
  a.full_resolution_depth = m->options.full_resolution_depth;
  a.linear_xy = s.linear_xy;
  a.linear_z = s.linear_z;
  a.min_score = min_score;
  return a;
}

// A search's packed chain output -> its score cache; returns theta.
float take_frontier(Search& s, const int* out, int out_records, int cap) {
  const int max_depth = s.m->max_depth();
  const FrontierRec* rec = reinterpret_cast<const FrontierRec*>(out + kMaxLevels + 2);
  int at = 0;
  for (int depth = max_depth; depth >= 0 && at < out_records; --depth) {
    const int cnt = std::min(std::min(out[depth], cap), out_records - at);
    for (int i = 0; i < cnt; ++i) s.cache.put(Search::key(depth, to_candidate(rec[at + i])), rec[at + i].sum);
    at += cnt;
  }
  s.scored += at;
  s.launches += max_depth + 3;
  float theta;
  std::memcpy(&theta, &out[kMaxLevels + 1], 4);
  s.frontier_threshold = theta;
  return theta;
}

// one wavefront per candidate: made for the clouds the reference matches (adaptive voxel filter, ~150-200 points);
// with every return of a scan (65 536 points) the single workgroup of step 2 alone takes 7 ms -- those searches keep
// the on-demand batches, whose block-per-chunk scoring kernel fills the chip
constexpr int kFrontierMaxPoints = 8192;
bool frontier_suits(const Search& s, size_t lowest, int cap) {
  const int max_depth = s.m->max_depth();
  return lowest > 0 && lowest <= static_cast<size_t>(cap) && max_depth + 1 <= kMaxLevels && max_depth >= 1 &&
         s.n_hi <= kFrontierMaxPoints;
}

// The single call's frontier: the chain with one search.  Does nothing (DLIOM_OK) for searches it is not made for;
// the recursion then fetches scores on demand.
int device_frontier(Search& s, const std::vector<Candidate>& lowest, float min_score) {
  dliom_ctx* ctx = s.ctx;
  const int max_depth = s.m->max_depth();
  constexpr int kCap = 8192;
  static_assert(frontier_upload_bytes(1, kCap) <= kPinFrontierUpload.bytes, "the largest upload fits its region");
  const size_t k = lowest.size();
  if (!frontier_suits(s, k, kCap)) return DLIOM_OK;
  const size_t up = align256(frontier_upload_bytes(1, k));
  const size_t pool_bytes = static_cast<size_t>(max_depth + 1) * kCap * sizeof(FrontierRec);
  DLIOM_TRY(ctx->cand.reserve(up + pool_bytes));
  char* d = static_cast<char*>(ctx->cand.p);
  char* h = pinned_at<char>(ctx, kPinFrontierUpload);
  int* out = pinned_at<int>(ctx, kPinFrontierOut);
  const int out_records = static_cast<int>((kPinFrontierOut.bytes - (kMaxLevels + 2) * 4) / sizeof(FrontierRec));
  FrontierArgs a = frontier_args(s, min_score);
  a.pool = reinterpret_cast<FrontierRec*>(d + up);
  a.counts = reinterpret_cast<int*>(d + frontier_counts_at(1));
  a.cap = kCap;
  a.top_begin = 0;
  a.top_count = static_cast<int>(k);
  a.out = out;
  a.out_records = out_records;
  std::memcpy(h, &a, sizeof(a));
  int* counts = reinterpret_cast<int*>(h + frontier_counts_at(1));
  std::memset(counts, 0, kCountWords * 4);
  counts[max_depth] = static_cast<int>(k);
  FrontierRec* flat = reinterpret_cast<FrontierRec*>(h + frontier_flat_at(1));
  for (size_t i = 0; i < k; ++i) flat[i] = to_rec(lowest[i]);
  DLIOM_HIP_TRY(hipMemcpyAsync(d, h, frontier_upload_bytes(1, k), hipMemcpyHostToDevice, ctx->stream));
  DLIOM_TRY(enqueue_frontier_chain(ctx, 1, static_cast<int>(k), max_depth, d));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  take_frontier(s, out, out_records, kCap);
  return DLIOM_OK;
}

PoseF pose_from_candidate(const Search& s, const Candidate& c) {  // :431-437
  const float r = s.m->resolution;
  const PoseF t{F3{r * static_cast<float>(c.offset[0]), r * static_cast<float>(c.offset[1]), r * static_cast<float>(c.offset[2])},
                QF{1.f, 0.f, 0.f, 0.f}};
  return pose_mul_f(t, s.scan_poses[c.scan_index]);
}

int low_resolution_score(Search& s, const Candidate& c, float* score) {  // low_resolution_matcher.cc:23-36
  float sum = 0.f;
  const auto ahead = s.low_sums.find(Search::key(0, c.scan_index, c.offset));
  if (ahead != s.low_sums.end()) {
    sum = ahead->second;  // scored by the batch's chain: the same kernels on the same pose
  } else {
    float p7[7];
    pose7(pose_from_candidate(s, c), p7);
    DLIOM_TRY(sequential_probability_sums(s.ctx, *s.lo_cloud, s.m->lo_grid, p7, 1, &sum));
  }
  *score = sum / static_cast<float>(s.lo_cloud->n);
  return DLIOM_OK;
}

// BranchAndBound (:439-492).  `status` carries device errors out of the recursion.
Candidate branch_and_bound(Search& s, const std::vector<Candidate>& candidates, int candidate_depth, float min_score,
                           int* status) {
  Candidate unsuccessful;
  unsuccessful.scan_index = 0;
  unsuccessful.offset[0] = unsuccessful.offset[1] = unsuccessful.offset[2] = 0;
  if (*status != DLIOM_OK) return unsuccessful;
  if (candidate_depth == 0) {
    for (const Candidate& c : candidates) {
      if (c.score <= min_score) return unsuccessful;
      float low = 0.f;
      *status = low_resolution_score(s, c, &low);
      if (*status != DLIOM_OK) return unsuccessful;
      if (low >= s.m->options.min_low_resolution_score) {
        Candidate best = c;
        best.low_resolution_score = low;
        return best;
      }
    }
    return unsuccessful;
  }
  Candidate best = unsuccessful;
  best.score = min_score;
  for (size_t i = 0; i < candidates.size(); ++i) {
    const Candidate& c = candidates[i];
    if (c.score <= min_score) break;
    std::vector<Candidate> higher;
    children_of(s, c, candidate_depth, &higher);
    if (!higher.empty() && !s.cache.has(Search::key(candidate_depth - 1, higher[0].scan_index, higher[0].offset))) {
      if (best.score > s.initial_min_score && best.score < s.frontier_threshold) {
        *status = prefetch_frontier(s, best.score);  // a match exists: everything still reachable, per level
        if (*status != DLIOM_OK) return unsuccessful;
      }
      if (!s.cache.has(Search::key(candidate_depth - 1, higher[0].scan_index, higher[0].offset))) {
        *status = prefetch_children(s, candidates, i, candidate_depth, best.score);
        if (*status != DLIOM_OK) return unsuccessful;
      }
    }
    *status = score_candidates(s, candidate_depth - 1, &higher);
    if (*status != DLIOM_OK) return unsuccessful;
    best = std::max(best, branch_and_bound(s, higher, candidate_depth - 1, best.score, status));
    if (*status != DLIOM_OK) return unsuccessful;
  }
  return best;
}

// Lowest-resolution candidates (:358-392, 419-429), or DLIOM_ERR_CAPACITY for searches that cannot fit.
int lowest_candidates(const Search& s, std::vector<Candidate>* lowest) {
  const int num_scans = static_cast<int>(s.scan_poses.size());
  const int step = 1 << s.m->max_depth();
  {
    // the reference would allocate them all as well; refuse searches that cannot fit instead of
    // exhausting host memory (a whole-submap window with a shallow pyramid is ~1e8 per scan)
    const double per_axis_xy = std::floor((2.0 * s.linear_xy + step) / step), per_axis_z = std::floor((2.0 * s.linear_z + step) / step);
    if (per_axis_xy * per_axis_xy * per_axis_z * num_scans > 3.0e7) return DLIOM_ERR_CAPACITY;
    // the score cache packs (depth, scan, offsets) into 64 bits: 14-bit offsets, 16-bit scan index (Search::key)
    if (s.linear_xy > 8191 || s.linear_z > 8191 || num_scans > 65535) return DLIOM_ERR_CAPACITY;
  }
  lowest->clear();
  for (int scan = 0; scan != num_scans; ++scan)
    for (int z = -s.linear_z; z <= s.linear_z; z += step)
      for (int y = -s.linear_xy; y <= s.linear_xy; y += step)
        for (int x = -s.linear_xy; x <= s.linear_xy; x += step) {
          Candidate c;
          c.scan_index = scan;
          c.offset[0] = x;
          c.offset[1] = y;
          c.offset[2] = z;
          lowest->push_back(c);
        }
  return DLIOM_OK;
}

// The recursion over a search whose discrete scans are on the device and whose cache holds what was fetched ahead.
int finish_search(Search& s, std::vector<Candidate>* lowest, float min_score, dliom_fast_csm_result* r) {
  DLIOM_TRY(score_candidates(s, s.m->max_depth(), lowest));
  s.top = lowest;
  s.initial_min_score = min_score;
  int status = DLIOM_OK;
  const Candidate best = branch_and_bound(s, *lowest, s.m->max_depth(), min_score, &status);
  DLIOM_TRY(status);
  r->num_scored_candidates = s.scored;
  r->num_score_launches = s.launches;
  if (best.score > min_score) {
    r->found = 1;
    r->score = best.score;
    pose7(pose_from_candidate(s, best), r->pose_estimate);
    r->rotational_score = s.rotational_scores[best.scan_index];
    r->low_resolution_score = best.low_resolution_score;
  }
  return DLIOM_OK;
}

int run_search(Search& s, const dliom_cloud& hi_cloud, float min_score, dliom_fast_csm_result* r) {
  const dliom_fast_csm* m = s.m;
  dliom_ctx* ctx = s.ctx;
  std::memset(r, 0, sizeof(*r));
  const int num_scans = static_cast<int>(s.scan_poses.size());
  r->num_discrete_scans = num_scans;
  if (num_scans == 0 || hi_cloud.n == 0) return DLIOM_OK;  // no candidates: nullptr in the reference
  s.n_hi = static_cast<int>(hi_cloud.n);
  // discrete scans on the device
  const size_t cells = static_cast<size_t>(num_scans) * s.n_hi;
  const size_t pose_bytes = align256(static_cast<size_t>(num_scans) * 28);
  DLIOM_TRY(ctx->sums.reserve(pose_bytes + 3 * cells * 4));
  float* d_poses = ctx->sums.as<float>();
  s.d_cx = reinterpret_cast<int*>(static_cast<char*>(ctx->sums.p) + pose_bytes);
  s.d_cy = s.d_cx + cells;
  s.d_cz = s.d_cy + cells;
  std::vector<float> poses(7 * static_cast<size_t>(num_scans));
  for (int i = 0; i < num_scans; ++i) pose7(s.scan_poses[i], &poses[7 * static_cast<size_t>(i)]);
  // through the pinned block when they fit: no synchronisation here, the stream orders the kernels behind the copy
  const bool poses_pinned = poses.size() * 4 <= kPinPoses.bytes;
  const float* poses_src = poses.data();
  if (poses_pinned) {
    float* staged = pinned_at<float>(ctx, kPinPoses);
    std::memcpy(staged, poses.data(), poses.size() * 4);
    poses_src = staged;
  }
  DLIOM_HIP_TRY(hipMemcpyAsync(d_poses, poses_src, poses.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(discretize_kernel, dim3((s.n_hi + 255) / 256, num_scans), dim3(256), 0, ctx->stream, hi_cloud.d_x,
                     hi_cloud.d_y, hi_cloud.d_z, s.n_hi, d_poses, m->resolution, s.d_cx, s.d_cy, s.d_cz);
  DLIOM_HIP_TRY(hipGetLastError());
  if (!poses_pinned) {  // pageable source
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    ++ctx->host_syncs;
  }
  std::vector<Candidate> lowest;
  DLIOM_TRY(lowest_candidates(s, &lowest));
  DLIOM_TRY(device_frontier(s, lowest, min_score));
  return finish_search(s, &lowest, min_score, r);
}

// GenerateDiscreteScans (:306-356): poses and rotational scores of the scans worth discretising.
void generate_discrete_scans(Search& s, const dliom_fast_csm_node_data& data, float max_norm, const PoseF& node,
                             const PoseF& submap) {
  const dliom_fast_csm* m = s.m;
  float max_scan_range = 3.f * m->resolution;
  max_scan_range = std::max(max_norm, max_scan_range);
  const float kSafetyMargin = 1.f - 1e-2f;
  const float res2 = m->resolution * m->resolution, range2 = max_scan_range * max_scan_range;
  const float angular_step_size = kSafetyMargin * std::acos(1.f - res2 / (2.f * range2));
  const int angular_window_size = static_cast<int>(std::lround(s.angular_window / angular_step_size));
  std::vector<float> angles;
  for (int rz = -angular_window_size; rz <= angular_window_size; ++rz) angles.push_back(rz * angular_step_size);
  const PoseF node_to_submap = pose_mul_f(pose_inverse_f(submap), node);
  // gravity_alignment.inverse() in double, then cast<float>()
  const double* g = data.gravity_alignment;
  const double n2 = (g[1] * g[1] + g[3] * g[3]) + (g[2] * g[2] + g[0] * g[0]);
  QF gi{0.f, 0.f, 0.f, 0.f};
  if (n2 > 0.) gi = QF{static_cast<float>(g[0] / n2), static_cast<float>(-g[1] / n2), static_cast<float>(-g[2] / n2),
                       static_cast<float>(-g[3] / n2)};
  const float initial_angle = get_yaw(qmul(node_to_submap.q, gi));
  const Histogram scan_histogram(data.rotational_scan_matcher_histogram,
                                 data.rotational_scan_matcher_histogram + m->submap_histogram.size());
  const QF submap_rotation_inverse = quat_inverse(submap.q);
  for (size_t i = 0; i != angles.size(); ++i) {
    const float score = match_histograms(m->submap_histogram, rotate_histogram(scan_histogram, initial_angle + angles[i]));
    if (score < m->options.min_rotational_score) continue;
    const QF yaw = angle_axis_to_quaternion(F3{0.f, 0.f, angles[i]});
    s.scan_poses.push_back(PoseF{node_to_submap.t, qmul(qmul(submap_rotation_inverse, yaw), node.q)});
    s.rotational_scores.push_back(score);
  }
}

PoseF to_pose_f(const double* p) {  // Rigid3d::cast<float>()
  return PoseF{F3{static_cast<float>(p[0]), static_cast<float>(p[1]), static_cast<float>(p[2])},
               QF{static_cast<float>(p[3]), static_cast<float>(p[4]), static_cast<float>(p[5]), static_cast<float>(p[6])}};
}

struct StagedClouds {
  dliom_cloud* hi = nullptr;
  dliom_cloud* lo = nullptr;
  ~StagedClouds() {
    if (hi) dliom_cloud_destroy(hi);
    if (lo) dliom_cloud_destroy(lo);
  }
};

bool valid_node_data(const dliom_fast_csm_node_data* data) {
  return !(data == nullptr || data->num_high_resolution_points < 0 || data->num_low_resolution_points <= 0 ||
           data->rotational_scan_matcher_histogram == nullptr ||
           (data->num_high_resolution_points > 0 && data->high_resolution_points == nullptr) ||
           data->low_resolution_points == nullptr);
}

int stage(dliom_ctx* ctx, const dliom_fast_csm_node_data* data, StagedClouds* c) {
  if (!valid_node_data(data)) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_TRY(dliom_cloud_create(ctx, data->high_resolution_points, data->num_high_resolution_points, &c->hi));
  DLIOM_TRY(dliom_cloud_create(ctx, data->low_resolution_points, data->num_low_resolution_points, &c->lo));
  return DLIOM_OK;
}

// The search of one call: window, discrete scans and their rotational scores.  Match (:147-165), MatchFullSubmap
// (:204-232; `pose` / `submap_pose` hold the rotations), MatchWith3DofInitial (:168-201).
void setup_search(Search* s, dliom_ctx* ctx, const dliom_fast_csm* m, int kind, const double* pose, const double* submap_pose,
                  const dliom_fast_csm_node_data& data, float max_norm) {
  s->m = m;
  s->ctx = ctx;
  if (kind == DLIOM_FAST_CSM_MATCH_FULL_SUBMAP) {
    const int w = (m->width_in_voxels + 1) / 2 + static_cast<int>(std::lround(max_norm / m->resolution + 0.5f));  // :209-216
    s->linear_xy = w;
    s->linear_z = w;
    s->angular_window = M_PI;
    const double node[7] = {0, 0, 0, pose[0], pose[1], pose[2], pose[3]};
    const double submap[7] = {0, 0, 0, submap_pose[0], submap_pose[1], submap_pose[2], submap_pose[3]};
    generate_discrete_scans(*s, data, max_norm, to_pose_f(node), to_pose_f(submap));
    return;
  }
  s->linear_xy = static_cast<int>(std::lround(m->options.linear_xy_search_window / m->resolution));  // :154-156
  s->linear_z = static_cast<int>(std::lround(m->options.linear_z_search_window / m->resolution));
  s->angular_window = m->options.angular_search_window;
  if (kind == DLIOM_FAST_CSM_MATCH) {
    generate_discrete_scans(*s, data, max_norm, to_pose_f(pose), to_pose_f(submap_pose));
  } else {
    s->scan_poses.push_back(to_pose_f(pose));  // :181-184
    s->rotational_scores.push_back(static_cast<float>(m->options.min_rotational_score + 0.01));
  }
}

// What the three single calls share.  `submap_pose` is neither read nor required by MatchWith3DofInitial.
int match_one(dliom_ctx* ctx, const dliom_fast_csm* m, int kind, const double* pose, const double* submap_pose,
              const dliom_fast_csm_node_data* data, float min_score, dliom_fast_csm_result* result) {
  if (ctx == nullptr || m == nullptr || pose == nullptr || result == nullptr ||
      (submap_pose == nullptr && kind != DLIOM_FAST_CSM_MATCH_WITH_3DOF_INITIAL))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (ctx->device != m->ctx->device) return DLIOM_ERR_INVALID_ARGUMENT;  // the pyramid lives on the creating device
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  StagedClouds c;
  DLIOM_TRY(stage(ctx, data, &c));
  Search s;
  setup_search(&s, ctx, m, kind, pose, submap_pose, *data, c.hi->max_norm);
  s.lo_cloud = c.lo;
  return run_search(s, *c.hi, min_score, result);
}

// ---- the batch (dliom_fast_csm_match_batch) -------------------------------------------------------------------
constexpr int kBatchCap = 4096;          // records per list of a batched search (the single call's: 8 192)
constexpr int kBatchOutRecords = 4096;   // records a batched search packs into its page-locked region
constexpr int kBatchLeavesAhead = 256;   // leaves per search whose low-resolution score the chain computes ahead
constexpr int kChunkSearches = 128;      // searches per chunk, and what bounds one chunk's scratch:
constexpr size_t kChunkTop = 1u << 18;   //   lowest-resolution candidates
constexpr size_t kChunkCellBytes = 256u << 20;  // discrete-scan cells
constexpr int kChunkScans = 65535;       //   discrete scans (discretize_batch_kernel's grid)

inline size_t pad64(int64_t n) { return (static_cast<size_t>(n) + 63) & ~static_cast<size_t>(63); }

// What one search takes of a chunk's blocks, each stated once: for the chunking (fast_csm_batch) and the layout below.
inline size_t num_scans_of(const Search& s) { return s.scan_poses.size(); }
inline size_t hi_cloud_bytes(const Search& s) { return align256(static_cast<size_t>(s.n_hi) * 12); }  // packed xyz
inline size_t lo_cloud_bytes(const Search& s) { return 3 * pad64(s.n_lo) * 4; }                       // SoA, zero padded
inline size_t pool_bytes(const Search& s) { return static_cast<size_t>(s.m->max_depth() + 1) * kBatchCap * sizeof(FrontierRec); }
inline size_t cell_bytes(const Search& s) { return align256(3 * num_scans_of(s) * static_cast<size_t>(s.n_hi) * 4); }

// One chunk's device block (ctx->batch) and page-locked block (ctx->batch_pinned), in the manner of pinned_layout.h.
// Device: the upload [frontier args | counts | flat top (frontier_*_at)][scans][hi][lo], then [pools][cells] and the leaves'
// [rot][trans][list][lsum].  Page-locked: the upload's mirror, then [h_out: out_stride per search][h_leaf: the mirror of
// rot, trans and list][h_lsum].  Within scans, hi, lo, pools and cells the searches follow one another in chunk order.
struct ChunkLayout {
  size_t total_top = 0, total_scans = 0;
  int deepest = 0, widest = 0;  // the deepest pyramid, the largest high-resolution cloud
  PinRegion scans, hi, lo, pools, cells, rot, trans, list, lsum, h_out, h_leaf, h_lsum;
  size_t out_stride, upload_bytes, device_bytes, pinned_bytes;
};
ChunkLayout chunk_layout(const int* ids, int S, const std::vector<std::unique_ptr<Search>>& searches,
                         const std::vector<std::vector<Candidate>>& lowest) {
  ChunkLayout L;
  size_t hi = 0, lo = 0, pool = 0, cells = 0;
  for (int j = 0; j < S; ++j) {
    const Search& s = *searches[ids[j]];
    L.total_top += lowest[ids[j]].size();
    L.total_scans += num_scans_of(s);
    hi += hi_cloud_bytes(s);
    lo += lo_cloud_bytes(s);
    pool += pool_bytes(s);
    cells += cell_bytes(s);
    L.deepest = std::max(L.deepest, s.m->max_depth());
    L.widest = std::max(L.widest, s.n_hi);
  }
  const size_t leaves = static_cast<size_t>(S) * kBatchLeavesAhead;
  L.out_stride = align256((kMaxLevels + 2) * 4 + static_cast<size_t>(kBatchOutRecords) * sizeof(FrontierRec));
  const auto end = [](PinRegion r) { return r.at + r.bytes; };
  const PinRegion front{0, align256(frontier_upload_bytes(S, L.total_top))};
  L.scans = PinRegion{end(front), align256(L.total_scans * sizeof(DiscreteScanArg))};
  L.hi = PinRegion{end(L.scans), hi};
  L.lo = PinRegion{end(L.hi), lo};
  L.upload_bytes = end(L.lo);
  L.pools = PinRegion{align256(L.upload_bytes), pool};
  L.cells = PinRegion{end(L.pools), cells};
  L.rot = PinRegion{end(L.cells), align256(leaves * 16)};
  L.trans = PinRegion{end(L.rot), align256(leaves * 12)};
  L.list = PinRegion{end(L.trans), align256(leaves * 4)};
  L.lsum = PinRegion{end(L.list), align256(leaves * 4)};
  L.device_bytes = end(L.lsum);
  L.h_out = PinRegion{align256(L.upload_bytes), S * L.out_stride};
  L.h_leaf = PinRegion{end(L.h_out), L.lsum.at - L.rot.at};
  L.h_lsum = PinRegion{end(L.h_leaf), L.lsum.bytes};
  L.pinned_bytes = end(L.h_lsum);
#ifdef DLIOM_DEBUG_CHECKS  // make experiments EXP_FLAGS=-DDLIOM_DEBUG_CHECKS; the shipped library has no abort path
  const auto chained = [&end](std::initializer_list<PinRegion> rs, size_t total) {  // no overlap, the last ends at the total
    size_t at = 0;
    for (const PinRegion& r : rs) {
      if (r.at < at) return false;
      at = end(r);
    }
    return at == total;
  };
  assert(chained({front, L.scans, L.hi, L.lo, L.pools, L.cells, L.rot, L.trans, L.list, L.lsum}, L.device_bytes));
  assert(chained({front, L.scans, L.hi, L.lo, L.h_out, L.h_leaf, L.h_lsum}, L.pinned_bytes));
#endif
  return L;
}

// One chunk: discretisation + frontier chain (one synchronisation), the low-resolution scores of the leaves at or
// above each search's theta (one more), then each search's recursion in query order.
int fast_csm_chunk(dliom_ctx* ctx, const dliom_fast_csm_query* queries, const int* ids, int S,
                   std::vector<std::unique_ptr<Search>>& searches, std::vector<std::vector<Candidate>>& lowest,
                   dliom_fast_csm_result* results, dliom_batch_stats* st) {
  const ChunkLayout L = chunk_layout(ids, S, searches, lowest);
  DLIOM_TRY(ctx->batch.reserve(L.device_bytes));
  DLIOM_TRY(ctx->reserve_batch_pinned(L.pinned_bytes));
  char* d = static_cast<char*>(ctx->batch.p);
  char* h = static_cast<char*>(ctx->batch_pinned);

  // ---- fill the upload
  FrontierArgs* h_args = reinterpret_cast<FrontierArgs*>(h);
  int* h_counts = reinterpret_cast<int*>(h + frontier_counts_at(S));
  FrontierRec* h_flat = reinterpret_cast<FrontierRec*>(h + frontier_flat_at(S));
  DiscreteScanArg* h_scans = reinterpret_cast<DiscreteScanArg*>(h + L.scans.at);
  std::memset(h_counts, 0, static_cast<size_t>(S) * kCountWords * 4);
  std::vector<dliom_cloud> lo(S);
  struct {
    size_t top = 0, scan = 0, hi = 0, lo = 0, pool = 0, cells = 0;
  } at;  // where search j begins in the flat top list, the scan arguments and (bytes) the regions of those names
  for (int j = 0; j < S; ++j) {
    Search& s = *searches[ids[j]];
    const dliom_fast_csm_node_data& nd = queries[ids[j]].node_data;
    const std::vector<Candidate>& low = lowest[ids[j]];
    const int num_scans = static_cast<int>(s.scan_poses.size());
    const size_t cells = static_cast<size_t>(num_scans) * s.n_hi;
    s.d_cx = reinterpret_cast<int*>(d + L.cells.at + at.cells);
    s.d_cy = s.d_cx + cells;
    s.d_cz = s.d_cy + cells;
    std::memcpy(h + L.hi.at + at.hi, nd.high_resolution_points, static_cast<size_t>(s.n_hi) * 12);
    for (int k = 0; k < num_scans; ++k) {
      DiscreteScanArg& a = h_scans[at.scan + k];
      a.pts = reinterpret_cast<const float*>(d + L.hi.at + at.hi);
      a.cx = s.d_cx + static_cast<size_t>(k) * s.n_hi;
      a.cy = s.d_cy + static_cast<size_t>(k) * s.n_hi;
      a.cz = s.d_cz + static_cast<size_t>(k) * s.n_hi;
      a.n = s.n_hi;
      a.resolution = s.m->resolution;
      pose7(s.scan_poses[k], a.pose);
    }
    // the low-resolution cloud, SoA, zero padded (what sequential_probability_sums reads of a dliom_cloud)
    const int64_t n_lo = nd.num_low_resolution_points;
    const size_t pl = pad64(n_lo);
    float* hx = reinterpret_cast<float*>(h + L.lo.at + at.lo);
    std::memset(hx, 0, lo_cloud_bytes(s));
    for (int64_t i = 0; i < n_lo; ++i) {
      hx[i] = nd.low_resolution_points[3 * i];
      hx[pl + i] = nd.low_resolution_points[3 * i + 1];
      hx[2 * pl + i] = nd.low_resolution_points[3 * i + 2];
    }
    dliom_cloud& c = lo[j];
    c.ctx = ctx;
    c.device = ctx->device;
    c.n = n_lo;
    c.n_padded = static_cast<int64_t>(pl);
    c.d_x = reinterpret_cast<float*>(d + L.lo.at + at.lo);
    c.d_y = c.d_x + pl;
    c.d_z = c.d_y + pl;
    c.max_norm = cloud_max_norm(nd.low_resolution_points, n_lo);
    c.owned_by_ctx_scratch = true;
    s.lo_cloud = &c;
    // the frontier
    FrontierArgs a = frontier_args(s, queries[ids[j]].min_score);
    a.pool = reinterpret_cast<FrontierRec*>(d + L.pools.at + at.pool);
    a.counts = reinterpret_cast<int*>(d + frontier_counts_at(S)) + static_cast<size_t>(j) * kCountWords;
    a.cap = kBatchCap;
    a.top_begin = static_cast<int>(at.top);
    a.top_count = static_cast<int>(low.size());
    a.out = reinterpret_cast<int*>(h + L.h_out.at + j * L.out_stride);
    a.out_records = kBatchOutRecords;
    std::memcpy(&h_args[j], &a, sizeof(a));
    h_counts[static_cast<size_t>(j) * kCountWords + a.max_depth] = a.top_count;
    for (size_t i = 0; i < low.size(); ++i) h_flat[at.top + i] = to_rec(low[i]);
    at.top += low.size();
    at.scan += num_scans_of(s);
    at.hi += hi_cloud_bytes(s);
    at.lo += lo_cloud_bytes(s);
    at.pool += pool_bytes(s);
    at.cells += cell_bytes(s);
  }
#ifdef DLIOM_DEBUG_CHECKS  // the searches filled each region exactly
  assert(at.top == L.total_top && at.scan == L.total_scans && at.hi == L.hi.bytes && at.lo == L.lo.bytes &&
         at.pool == L.pools.bytes && at.cells == L.cells.bytes);
#endif

  // ---- one upload, the discrete scans, the chain, one synchronisation
  DLIOM_HIP_TRY(hipMemcpyAsync(d, h, L.upload_bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(discretize_batch_kernel, dim3(static_cast<unsigned>((L.widest + 255) / 256), static_cast<unsigned>(L.total_scans)),
                     dim3(256), 0, ctx->stream, reinterpret_cast<const DiscreteScanArg*>(d + L.scans.at));
  DLIOM_TRY(enqueue_frontier_chain(ctx, S, static_cast<int>(L.total_top), L.deepest, d));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  ++ctx->host_syncs;
  ++st->chunks;
  ++st->frontier_chains;

  // ---- the leaves at or above theta: their low-resolution sums, ahead of the recursion (one more synchronisation)
  float4* h_rot = reinterpret_cast<float4*>(h + L.h_leaf.at);
  float* h_trans = reinterpret_cast<float*>(h + L.h_leaf.at + (L.trans.at - L.rot.at));
  unsigned* h_list = reinterpret_cast<unsigned*>(h + L.h_leaf.at + (L.list.at - L.rot.at));
  std::vector<SequentialSumJob> jobs;
  std::vector<std::vector<uint64_t>> leaf_keys(S);
  int first = 0;
  for (int j = 0; j < S; ++j) {
    Search& s = *searches[ids[j]];
    const int* out = reinterpret_cast<const int*>(h + L.h_out.at + j * L.out_stride);
    const float theta = take_frontier(s, out, kBatchOutRecords, kBatchCap);
    const float min_score = queries[ids[j]].min_score;
    int at = 0;  // the depth-0 records come last
    for (int depth = s.m->max_depth(); depth >= 1; --depth) at += std::min(out[depth], kBatchCap);
    const int end = std::min(at + std::min(out[0], kBatchCap), kBatchOutRecords);
    const FrontierRec* rec = reinterpret_cast<const FrontierRec*>(out + kMaxLevels + 2);
    int k = 0;
    for (int i = at; i < end && k < kBatchLeavesAhead; ++i) {
      const Candidate c = to_candidate(rec[i]);
      const float score = to_probability(rec[i].sum / static_cast<float>(s.n_hi));
      if (!(score >= theta && score > min_score)) continue;
      const PoseF p = pose_from_candidate(s, c);
      h_rot[first + k] = make_float4(p.q.w, p.q.x, p.q.y, p.q.z);
      h_trans[3 * (first + k)] = p.t.x;
      h_trans[3 * (first + k) + 1] = p.t.y;
      h_trans[3 * (first + k) + 2] = p.t.z;
      leaf_keys[j].push_back(Search::key(0, c));
      ++k;
    }
    for (int i = 0; i < k; ++i) h_list[first + i] = static_cast<unsigned>(i * k + i);
    if (k > 0) jobs.push_back(SequentialSumJob{s.lo_cloud, s.m->lo_grid, first, k});
    first += k;
  }
  if (first > 0) {
    DLIOM_HIP_TRY(hipMemcpyAsync(d + L.rot.at, h + L.h_leaf.at, L.h_leaf.bytes, hipMemcpyHostToDevice, ctx->stream));
    float* d_lsum = reinterpret_cast<float*>(d + L.lsum.at);
    DLIOM_TRY(sequential_probability_sums_enqueue(ctx, jobs.data(), static_cast<int>(jobs.size()),
                                                  reinterpret_cast<const float4*>(d + L.rot.at),
                                                  reinterpret_cast<const float*>(d + L.trans.at),
                                                  reinterpret_cast<const unsigned*>(d + L.list.at), d_lsum));
    float* h_lsum = reinterpret_cast<float*>(h + L.h_lsum.at);
    DLIOM_HIP_TRY(hipMemcpyAsync(h_lsum, d_lsum, static_cast<size_t>(first) * 4, hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    ++ctx->host_syncs;
    int at = 0;
    for (int j = 0; j < S; ++j)
      for (uint64_t key : leaf_keys[j]) searches[ids[j]]->low_sums[key] = h_lsum[at++];
  }

  // ---- the recursions, in query order
  for (int j = 0; j < S; ++j) {
    Search& s = *searches[ids[j]];
    DLIOM_TRY(finish_search(s, &lowest[ids[j]], queries[ids[j]].min_score, &results[ids[j]]));
    st->cache_misses += s.cache_misses;
    s.lo_cloud = nullptr;  // lo[] ends with this chunk
  }
  st->batched += S;
  return DLIOM_OK;
}

int fast_csm_batch(dliom_ctx* ctx, const dliom_fast_csm_query* queries, int count, dliom_fast_csm_result* results,
                   int* statuses, dliom_batch_stats* st) {
  std::vector<std::unique_ptr<Search>> searches(count);
  std::vector<std::vector<Candidate>> lowest(count);
  std::vector<int> batched;
  for (int i = 0; i < count; ++i) {  // host preparation; the single calls for what the chain is not made for
    const dliom_fast_csm_query& q = queries[i];
    const dliom_fast_csm_node_data& nd = q.node_data;
    dliom_fast_csm_result* r = &results[i];
    std::memset(r, 0, sizeof(*r));
    statuses[i] = DLIOM_OK;
    std::unique_ptr<Search> s(new Search);
    setup_search(s.get(), ctx, q.matcher, q.kind, q.pose, q.submap_pose, nd,
                 cloud_max_norm(nd.high_resolution_points, nd.num_high_resolution_points));
    r->num_discrete_scans = static_cast<int>(s->scan_poses.size());
    if (s->scan_poses.empty() || nd.num_high_resolution_points == 0) {  // no candidates: nullptr in the reference
      ++st->without_search;
      continue;
    }
    s->n_hi = static_cast<int>(nd.num_high_resolution_points);
    s->n_lo = nd.num_low_resolution_points;
    statuses[i] = lowest_candidates(*s, &lowest[i]);
    if (statuses[i] != DLIOM_OK) {
      ++st->without_search;
      continue;
    }
    if (!frontier_suits(*s, lowest[i].size(), kBatchCap)) {
      const int status = match_one(ctx, q.matcher, q.kind, q.pose, q.submap_pose, &nd, q.min_score, r);
      if (status != DLIOM_OK && status != DLIOM_ERR_CAPACITY) return status;
      statuses[i] = status;
      lowest[i].clear();
      ++st->per_query;
      ++st->per_query_frontier;
      continue;
    }
    searches[i] = std::move(s);
    batched.push_back(i);
  }
  for (size_t at = 0; at < batched.size();) {
    size_t end = at, top = 0, cells = 0;
    int scans = 0;
    while (end < batched.size() && end - at < static_cast<size_t>(kChunkSearches)) {
      const Search& s = *searches[batched[end]];
      const size_t k = lowest[batched[end]].size(), c = cell_bytes(s);
      const int ns = static_cast<int>(num_scans_of(s));
      if (end > at && (top + k > kChunkTop || cells + c > kChunkCellBytes || scans + ns > kChunkScans)) break;
      top += k;
      cells += c;
      scans += ns;
      ++end;
    }
    DLIOM_TRY(fast_csm_chunk(ctx, queries, &batched[at], static_cast<int>(end - at), searches, lowest, results, st));
    for (size_t j = at; j < end; ++j) {  // done: free the host side early
      searches[batched[j]].reset();
      std::vector<Candidate>().swap(lowest[batched[j]]);
    }
    at = end;
  }
  return DLIOM_OK;
}

}  // namespace

extern "C" {

int dliom_fast_csm_create(dliom_ctx* ctx, const dliom_grid* hi, const dliom_grid* lo, const float* node_histograms,
                          const float* node_angles, int num_nodes, int histogram_size,
                          const dliom_fast_csm_options* o, dliom_fast_csm** out) {
  if (ctx == nullptr || hi == nullptr || lo == nullptr || o == nullptr || out == nullptr || num_nodes <= 0 ||
      histogram_size <= 0 || node_histograms == nullptr || node_angles == nullptr)
    return DLIOM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (o->branch_and_bound_depth < 1 || o->full_resolution_depth < 1 || o->branch_and_bound_depth > 15)
    return DLIOM_ERR_INVALID_ARGUMENT;  // CHECK_GE(depth, 1) (:60-61)
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<dliom_fast_csm> m(new dliom_fast_csm);
  m->ctx = ctx;
  m->options = *o;
  m->resolution = hi->resolution;
  m->width_in_voxels = 64 << hi->bits;
  m->lo_grid = lo;
  // RotationalScanMatcher ctor (:174-182)
  m->submap_histogram.assign(histogram_size, 0.f);
  for (int k = 0; k < num_nodes; ++k) {
    const Histogram h(node_histograms + static_cast<size_t>(k) * histogram_size,
                      node_histograms + static_cast<size_t>(k + 1) * histogram_size);
    const Histogram r = rotate_histogram(h, node_angles[k]);
    for (int i = 0; i < histogram_size; ++i) m->submap_histogram[i] += r[i];
  }
  // level 0 over the bounding box of the leaves
  int64_t count = 0;
  DLIOM_TRY(const_cast<dliom_grid*>(hi)->refresh_count(&count));
  m->levels.resize(o->branch_and_bound_depth);
  if (count > 1) {
    DLIOM_TRY(ctx->misc.reserve(32768 + 64));
    int* d_mm = reinterpret_cast<int*>(static_cast<char*>(ctx->misc.p) + 32768);
    const int init[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
    DLIOM_HIP_TRY(hipMemcpyAsync(d_mm, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(leaf_bbox_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, ctx->stream,
                       hi->d_slot_coord, static_cast<unsigned>(count), d_mm);
    int mm[6];
    DLIOM_HIP_TRY(hipMemcpyAsync(mm, d_mm, sizeof(mm), hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    // ConvertToPrecomputationGrid's value map (:53-57), host float arithmetic like the reference
    std::vector<uint8_t> lut(32768, 0);
    for (int v = 1; v < 32768; ++v) {
      const long cell = std::lround((value_to_probability(v) - kMinProbability) * (255.f / (kMaxProbability - kMinProbability)));
      lut[v] = static_cast<uint8_t>(std::min(255l, std::max(0l, cell)));
    }
    uint8_t* d_lut = static_cast<uint8_t*>(ctx->misc.p);
    DLIOM_HIP_TRY(hipMemcpyAsync(d_lut, lut.data(), 32768, hipMemcpyHostToDevice, ctx->stream));
    dliom_fast_csm::Level& l0 = m->levels[0];
    for (int a = 0; a < 3; ++a) {
      l0.lo[a] = mm[a] * 8;
      l0.n[a] = (mm[3 + a] - mm[a] + 1) * 8;
    }
    DLIOM_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&l0.d), l0.cells()));
    DLIOM_HIP_TRY(hipMemsetAsync(l0.d, 0, l0.cells(), ctx->stream));
    hipLaunchKernelGGL(convert_level0_kernel, dim3(static_cast<unsigned>(count - 1)), dim3(256), 0, ctx->stream,
                       hi->d_slot_coord, hi->d_pool, d_lut, l0.d, l0.lo[0], l0.lo[1], l0.lo[2], l0.n[0], l0.n[1]);
    DLIOM_HIP_TRY(hipGetLastError());
    int last_width = 1;
    for (int depth = 1; depth != o->branch_and_bound_depth; ++depth) {  // :65-76
      const bool half = depth >= o->full_resolution_depth;
      const int next_width = 1 << depth;
      const int per_high = 1 << std::max(0, depth - o->full_resolution_depth);
      const int shift = (next_width - last_width + (per_high - 1)) / per_high;
      const dliom_fast_csm::Level& src = m->levels[depth - 1];
      dliom_fast_csm::Level& dst = m->levels[depth];
      for (int a = 0; a < 3; ++a) {
        const int lo_c = src.lo[a] - shift, hi_c = src.lo[a] + src.n[a] - 1;
        dst.lo[a] = half ? (lo_c >> 1) : lo_c;
        dst.n[a] = (half ? (hi_c >> 1) : hi_c) - dst.lo[a] + 1;
      }
      DLIOM_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dst.d), dst.cells()));
      hipLaunchKernelGGL(precompute_level_kernel, dim3(static_cast<unsigned>((dst.cells() + 255) / 256)), dim3(256), 0,
                         ctx->stream, src.view(), dst.d, dst.lo[0], dst.lo[1], dst.lo[2], dst.n[0], dst.n[1], dst.n[2],
                         shift, half ? 1 : 0);
      DLIOM_HIP_TRY(hipGetLastError());
      last_width = next_width;
    }
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  *out = m.release();
  return DLIOM_OK;
}

int dliom_fast_csm_destroy(dliom_fast_csm* m) {
  if (m == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  (void)hipDeviceSynchronize();
  delete m;
  return DLIOM_OK;
}

int dliom_fast_csm_level(const dliom_fast_csm* m, int depth, int32_t lo[3], int32_t dims[3], uint8_t* values,
                         int64_t capacity) {
  if (m == nullptr || lo == nullptr || dims == nullptr || depth < 0 || depth > m->max_depth())
    return DLIOM_ERR_INVALID_ARGUMENT;
  const dliom_fast_csm::Level& l = m->levels[depth];
  for (int a = 0; a < 3; ++a) {
    lo[a] = l.lo[a];
    dims[a] = l.n[a];
  }
  if (values != nullptr) {
    if (capacity < static_cast<int64_t>(l.cells())) return DLIOM_ERR_CAPACITY;
    if (l.cells() > 0) DLIOM_HIP_TRY(hipMemcpy(values, l.d, l.cells(), hipMemcpyDeviceToHost));
  }
  return DLIOM_OK;
}

int dliom_fast_csm_match(dliom_ctx* ctx, const dliom_fast_csm* m, const double global_node_pose[7], const double global_submap_pose[7],
                         const dliom_fast_csm_node_data* data, float min_score, dliom_fast_csm_result* result) {
  return match_one(ctx, m, DLIOM_FAST_CSM_MATCH, global_node_pose, global_submap_pose, data, min_score, result);
}

int dliom_fast_csm_match_full_submap(dliom_ctx* ctx, const dliom_fast_csm* m, const double global_node_rotation[4],
                                     const double global_submap_rotation[4], const dliom_fast_csm_node_data* data,
                                     float min_score, dliom_fast_csm_result* result) {
  return match_one(ctx, m, DLIOM_FAST_CSM_MATCH_FULL_SUBMAP, global_node_rotation, global_submap_rotation, data, min_score, result);
}

int dliom_fast_csm_match_with_3dof_initial(dliom_ctx* ctx, const dliom_fast_csm* m, const double pose_in_submap_guess[7],
                                           const dliom_fast_csm_node_data* data, float min_score,
                                           dliom_fast_csm_result* result) {
  return match_one(ctx, m, DLIOM_FAST_CSM_MATCH_WITH_3DOF_INITIAL, pose_in_submap_guess, nullptr, data, min_score, result);
}

int dliom_fast_csm_match_batch(dliom_ctx* ctx, const dliom_fast_csm_query* queries, int count, dliom_fast_csm_result* results,
                               int* statuses, dliom_batch_stats* stats) {
  if (ctx == nullptr || count < 0 || (count > 0 && (queries == nullptr || results == nullptr || statuses == nullptr)))
    return DLIOM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < count; ++i) {
    const dliom_fast_csm_query& q = queries[i];
    if (q.matcher == nullptr || q.kind < DLIOM_FAST_CSM_MATCH || q.kind > DLIOM_FAST_CSM_MATCH_WITH_3DOF_INITIAL ||
        q.matcher->ctx->device != ctx->device || q.histogram_size != static_cast<int>(q.matcher->submap_histogram.size()) ||
        !valid_node_data(&q.node_data))
      return DLIOM_ERR_INVALID_ARGUMENT;
  }
  dliom_batch_stats st;
  std::memset(&st, 0, sizeof(st));
  const int64_t read_backs0 = ctx->read_backs, syncs0 = ctx->host_syncs;
  if (count > 0) {
    DLIOM_HIP_TRY(hipSetDevice(ctx->device));
    DLIOM_TRY(fast_csm_batch(ctx, queries, count, results, statuses, &st));
  }
  st.synchronizations = ctx->host_syncs - syncs0;
  st.read_backs = ctx->read_backs - read_backs0;
  if (stats != nullptr) *stats = st;
  return DLIOM_OK;
}

}  // extern "C"
