// Submap feature matching (dliom.h "submap feature matching"): the second half of
// ConstraintBuilder3D::ExtractFeaturesForSubmap (constraint_builder_3d.cc:459-529) on stored sets of key points and
// descriptors.  The definition -- the pinned fmaf chain of the distances, the ratio test, the hypotheses, the inlier
// test and the refit -- is stated once, in the header; the kernels below follow it operation for operation (this file
// is built with -ffp-contract=off and correctly rounded sqrtf like every other).
//
//   feature_knn_kernel     one workgroup per (tile of 256 queries, train set): a lane keeps its query descriptor in
//                          registers, the train set streams through LDS in chunks that every lane reads at the same
//                          address (a broadcast), each lane runs the fmaf chain and keeps (s0, j0, s1, j1)
//   feature_good_kernel    one workgroup per train set: ratio test, stable compaction (ballot + prefix), float points
//   feature_ransac_kernel  one workgroup per train set that reached minimum_good_match_num: points in LDS, a lane takes
//                          hypotheses h, h + 256, ...; integer inlier counts; one 64-bit max of (count + 1, ~h); one
//                          wave makes the winner's inlier mask, one lane the sequential refit sums
//   feature_readback_kernel copies the 48-byte records into the page-locked block and writes the completion word
//
// Every train set of a call has the same query set, so the grid is (tile, set) and a set's outputs start at set * nq:
// the table the kernels read holds the sets' pointers, sizes and image corners.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>

#include "internal.h"

namespace dliom {
namespace {

constexpr int kKnnThreads = 256;  // 4 waves: a tile of 256 queries
constexpr int kRansacThreads = 256;
constexpr int kChunk = DLIOM_FEATURE_TRAIN_CHUNK;
constexpr int kMaxGood = DLIOM_FEATURE_MAX_GOOD;

struct FeaturePair {  // 32 bytes (kPinFeaturePairs)
  const float* descriptors;  // the train set's, nt x D
  const float* keypoints;    // nt x 2
  int nt;                    // 0: the pair is not matched (a set with fewer than two key points)
  float ox, oy;              // (float)ox_t, (float)oy_t
  int pad;
};
static_assert(sizeof(FeaturePair) == 32, "kPinFeaturePairs holds 32 bytes a train set");

struct RansacRecord {  // 48 bytes (kPinFeatureResults)
  int good, inliers, hypothesis, flags;
  double a, b, tx, ty;
};
static_assert(sizeof(RansacRecord) == 48, "kPinFeatureResults holds 48 bytes a train set");
enum : int { kFlagEvaluated = 1, kFlagNoModel = 2, kFlagCapacity = 4 };

// ---- nearest neighbours --------------------------------------------------------------------------------------------
// DP: the descriptor size rounded up to 16 / 32 / 64 / 128.  The dimensions D .. DP-1 hold 0 on both sides:
// fmaf(0, 0, s) == s for every s >= 0, so the padded chain gives the bits of the chain over D.
template <int DP>
__global__ __launch_bounds__(kKnnThreads) void feature_knn_kernel(const float* __restrict__ query, int nq, int D,
                                                                  const FeaturePair* __restrict__ pairs, int* __restrict__ out_j0,
                                                                  int* __restrict__ out_j1, float* __restrict__ out_d0,
                                                                  float* __restrict__ out_d1) {
  constexpr int V = DP / 4;
  __shared__ float4 chunk[kChunk * V];
  const FeaturePair pair = pairs[blockIdx.y];
  if (pair.nt < 2) return;  // the whole workgroup
  const int i = blockIdx.x * kKnnThreads + threadIdx.x;
  float4 q[V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    q[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < nq && 4 * c < D) q[c] = *reinterpret_cast<const float4*>(query + static_cast<size_t>(i) * D + 4 * c);
  }
  const float inf = __int_as_float(0x7f800000);
  float s0 = inf, s1 = inf;
  int j0 = -1, j1 = -1;
  for (int base = 0; base < pair.nt; base += kChunk) {
    const int rows = min(kChunk, pair.nt - base);
    __syncthreads();
    for (int e = threadIdx.x; e < rows * V; e += kKnnThreads) {
      const int r = e / V, c = e % V;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (4 * c < D) t = *reinterpret_cast<const float4*>(pair.descriptors + static_cast<size_t>(base + r) * D + 4 * c);
      chunk[e] = t;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const float4 t = chunk[r * V + c];  // one address for the whole wave
        float diff = q[c].x - t.x;
        s = fmaf(diff, diff, s);
        diff = q[c].y - t.y;
        s = fmaf(diff, diff, s);
        diff = q[c].z - t.z;
        s = fmaf(diff, diff, s);
        diff = q[c].w - t.w;
        s = fmaf(diff, diff, s);
      }
      const int j = base + r;
      // ascending j and strict comparisons: ties go to the lowest j.  The index tests make the first two candidates
      // enter whatever their s (a sum that overflowed to +inf is still a least one).
      if (s < s0 || j0 < 0) {
        s1 = s0;
        j1 = j0;
        s0 = s;
        j0 = j;
      } else if (s < s1 || j1 < 0) {
        s1 = s;
        j1 = j;
      }
    }
  }
  if (i < nq) {
    const size_t at = static_cast<size_t>(blockIdx.y) * nq + i;
    out_j0[at] = j0;
    out_j1[at] = j1;
    out_d0[at] = sqrtf(s0);
    out_d1[at] = sqrtf(s1);
  }
}

// ---- good matches --------------------------------------------------------------------------------------------------
// points[set * stride + m] = (from.x, from.y, to.x, to.y) of the set's m-th good match, m < stride; counts[set] counts
// them all, also those beyond the stride
__global__ __launch_bounds__(256) void feature_good_kernel(const float* __restrict__ query_keypoints, int nq, float qox, float qoy,
                                                           double resolution, double ratio, const FeaturePair* __restrict__ pairs,
                                                           const int* __restrict__ j0, const float* __restrict__ d0,
                                                           const float* __restrict__ d1, float4* __restrict__ points, int stride,
                                                           int* __restrict__ counts) {
  __shared__ int wave_total[4];
  const FeaturePair pair = pairs[blockIdx.x];
  if (pair.nt < 2) {
    if (threadIdx.x == 0) counts[blockIdx.x] = 0;
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t first = static_cast<size_t>(blockIdx.x) * nq;
  int running = 0;
  for (int base = 0; base < nq; base += 256) {
    const int i = base + threadIdx.x;
    bool good = false;
    int j = 0;
    if (i < nq) {
      good = static_cast<double>(d0[first + i]) < ratio * static_cast<double>(d1[first + i]);
      j = j0[first + i];
    }
    const unsigned long long votes = __ballot(good);
    if (lane == 0) wave_total[wave] = __popcll(votes);
    __syncthreads();
    int at = running + __popcll(votes & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) at += wave_total[w];
    running += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    if (good && at < stride) {
      const float fx = qox + static_cast<float>(static_cast<double>(query_keypoints[2 * i]) * resolution);
      const float fy = qoy + static_cast<float>(static_cast<double>(query_keypoints[2 * i + 1]) * resolution);
      const float tx = pair.ox + static_cast<float>(static_cast<double>(pair.keypoints[2 * j]) * resolution);
      const float ty = pair.oy + static_cast<float>(static_cast<double>(pair.keypoints[2 * j + 1]) * resolution);
      points[static_cast<size_t>(blockIdx.x) * stride + at] = make_float4(fx, fy, tx, ty);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = running;
}

// ---- hypotheses and refit ------------------------------------------------------------------------------------------
struct Similarity {
  double a, b, tx, ty;
};

__device__ inline void hypothesis_matches(int M, bool enumerated, unsigned long long seed, int h, int* i, int* j) {
  if (enumerated) {  // all pairs i < j in lexicographic order: row i holds M - 1 - i of them
    int row = 0, rest = h;
    while (rest >= M - 1 - row) {
      rest -= M - 1 - row;
      ++row;
    }
    *i = row;
    *j = row + 1 + rest;
    return;
  }
  unsigned long long z = seed + static_cast<unsigned long long>(h);
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const unsigned a = static_cast<unsigned>(z) % static_cast<unsigned>(M);
  unsigned b = static_cast<unsigned>(z >> 32) % static_cast<unsigned>(M - 1);
  b += b >= a ? 1u : 0u;
  *i = static_cast<int>(a);
  *j = static_cast<int>(b);
}

// false: degenerate
__device__ inline bool similarity_of(const float4 pi, const float4 pj, Similarity* m) {
  const double pix = pi.x, piy = pi.y, Pix = pi.z, Piy = pi.w;
  const double dx = static_cast<double>(pj.x) - pix, dy = static_cast<double>(pj.y) - piy;
  const double ex = static_cast<double>(pj.z) - Pix, ey = static_cast<double>(pj.w) - Piy;
  const double den = dx * dx + dy * dy;
  if (den == 0.0) return false;
  m->a = (dx * ex + dy * ey) / den;
  m->b = (dx * ey - dy * ex) / den;
  m->tx = Pix - (m->a * pix - m->b * piy);
  m->ty = Piy - (m->b * pix + m->a * piy);
  return true;
}

__device__ inline bool is_inlier(const Similarity& m, const float4 pk, double threshold_squared) {
  const double px = pk.x, py = pk.y;
  const double rx = ((m.a * px - m.b * py) + m.tx) - static_cast<double>(pk.z);
  const double ry = ((m.b * px + m.a * py) + m.ty) - static_cast<double>(pk.w);
  return rx * rx + ry * ry <= threshold_squared;
}

// counts == nullptr: every workgroup has fixed_count matches (the diagnostic).  mask (may be null): stride bytes a set.
__global__ __launch_bounds__(kRansacThreads) void feature_ransac_kernel(const float4* __restrict__ points, int stride,
                                                                        const int* __restrict__ counts, int fixed_count,
                                                                        int minimum_good, double threshold_squared,
                                                                        unsigned long long seed, RansacRecord* __restrict__ records,
                                                                        unsigned char* __restrict__ mask) {
  extern __shared__ float4 pts[];  // stride points
  __shared__ unsigned char inlier[kMaxGood];
  __shared__ unsigned long long wave_best[kRansacThreads / 64];
  const int M = counts != nullptr ? counts[blockIdx.x] : fixed_count;
  RansacRecord rec = {M, 0, -1, 0, 0.0, 0.0, 0.0, 0.0};
  unsigned char* const my_mask = mask != nullptr ? mask + static_cast<size_t>(blockIdx.x) * stride : nullptr;
  if (M < minimum_good || M > stride || M > kMaxGood) {  // the whole workgroup
    if (M >= minimum_good) rec.flags = kFlagCapacity;
    if (threadIdx.x == 0) records[blockIdx.x] = rec;
    return;
  }
  for (int k = threadIdx.x; k < M; k += kRansacThreads) {
    pts[k] = points[static_cast<size_t>(blockIdx.x) * stride + k];
    if (my_mask != nullptr) my_mask[k] = 0;
  }
  __syncthreads();
  const int all_pairs = M * (M - 1) / 2;  // M <= 4096
  const bool enumerated = all_pairs <= DLIOM_FEATURE_RANSAC_HYPOTHESES;
  const int num_hypotheses = M < 2 ? 0 : (enumerated ? all_pairs : DLIOM_FEATURE_RANSAC_HYPOTHESES);
  unsigned long long best = 0;  // (inliers + 1) << 32 | ~h; 0: degenerate or none
  for (int h = threadIdx.x; h < num_hypotheses; h += kRansacThreads) {
    int i, j;
    hypothesis_matches(M, enumerated, seed, h, &i, &j);
    Similarity m;
    if (!similarity_of(pts[i], pts[j], &m)) continue;
    unsigned count = 0;
    for (int k = 0; k < M; ++k) count += is_inlier(m, pts[k], threshold_squared) ? 1u : 0u;
    const unsigned long long key = (static_cast<unsigned long long>(count + 1u) << 32) | (0xFFFFFFFFu - static_cast<unsigned>(h));
    best = key > best ? key : best;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(best, off);
    best = other > best ? other : best;
  }
  if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
  __syncthreads();
  best = wave_best[0];
  for (int w = 1; w < kRansacThreads / 64; ++w) best = wave_best[w] > best ? wave_best[w] : best;
  rec.flags = kFlagEvaluated;
  if (best == 0) {
    rec.flags |= kFlagNoModel;
    if (threadIdx.x == 0) records[blockIdx.x] = rec;
    return;
  }
  const int h = static_cast<int>(0xFFFFFFFFu - static_cast<unsigned>(best & 0xFFFFFFFFull));
  int bi, bj;
  hypothesis_matches(M, enumerated, seed, h, &bi, &bj);
  Similarity m;
  (void)similarity_of(pts[bi], pts[bj], &m);
  if (threadIdx.x < 64) {
    for (int k = threadIdx.x; k < M; k += 64) {
      const unsigned char in = is_inlier(m, pts[k], threshold_squared) ? 1 : 0;
      inlier[k] = in;
      if (my_mask != nullptr) my_mask[k] = in;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  // the refit: sequential sums in match order
  int n = 0;
  double spx = 0.0, spy = 0.0, sPx = 0.0, sPy = 0.0;
  for (int k = 0; k < M; ++k) {
    if (!inlier[k]) continue;
    const float4 p = pts[k];
    ++n;
    spx += static_cast<double>(p.x);
    spy += static_cast<double>(p.y);
    sPx += static_cast<double>(p.z);
    sPy += static_cast<double>(p.w);
  }
  const double count = static_cast<double>(n);
  const double mpx = spx / count, mpy = spy / count, mPx = sPx / count, mPy = sPy / count;
  double sdd = 0.0, sde = 0.0, sx = 0.0;
  for (int k = 0; k < M; ++k) {
    if (!inlier[k]) continue;
    const float4 p = pts[k];
    const double dcx = static_cast<double>(p.x) - mpx, dcy = static_cast<double>(p.y) - mpy;
    const double ecx = static_cast<double>(p.z) - mPx, ecy = static_cast<double>(p.w) - mPy;
    sdd += dcx * dcx + dcy * dcy;
    sde += dcx * ecx + dcy * ecy;
    sx += dcx * ecy - dcy * ecx;
  }
  if (sdd != 0.0) {
    m.a = sde / sdd;
    m.b = sx / sdd;
    m.tx = mPx - (m.a * mpx - m.b * mpy);
    m.ty = mPy - (m.b * mpx + m.a * mpy);
  }
  rec.inliers = n;
  rec.hypothesis = h;
  rec.a = m.a;
  rec.b = m.b;
  rec.tx = m.tx;
  rec.ty = m.ty;
  records[blockIdx.x] = rec;
}

// the call's one read-back: the records into the page-locked block, then the completion word (as gather_to_pinned)
__global__ __launch_bounds__(1024) void feature_readback_kernel(const unsigned* __restrict__ src, unsigned words, unsigned* dst,
                                                                unsigned* done_word, unsigned done_seq) {
  for (unsigned w = threadIdx.x; w < words; w += 1024) dst[w] = src[w];
  if (done_word != nullptr) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence_system();
      *reinterpret_cast<volatile unsigned*>(done_word) = done_seq;
    }
  }
}

int launch_knn(hipStream_t stream, int D, const float* query, int nq, const FeaturePair* pairs, int num_pairs, int* j0, int* j1,
               float* d0, float* d1) {
  const dim3 grid(blocks_of(nq, kKnnThreads), static_cast<unsigned>(num_pairs));
  if (D <= 16)
    hipLaunchKernelGGL(feature_knn_kernel<16>, grid, dim3(kKnnThreads), 0, stream, query, nq, D, pairs, j0, j1, d0, d1);
  else if (D <= 32)
    hipLaunchKernelGGL(feature_knn_kernel<32>, grid, dim3(kKnnThreads), 0, stream, query, nq, D, pairs, j0, j1, d0, d1);
  else if (D <= 64)
    hipLaunchKernelGGL(feature_knn_kernel<64>, grid, dim3(kKnnThreads), 0, stream, query, nq, D, pairs, j0, j1, d0, d1);
  else
    hipLaunchKernelGGL(feature_knn_kernel<128>, grid, dim3(kKnnThreads), 0, stream, query, nq, D, pairs, j0, j1, d0, d1);
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

// the RANSAC kernel's points: dynamic LDS beyond the 64 KiB a kernel gets unasked (4 KiB of it is the static mask)
int launch_ransac(dliom_ctx* ctx, const float4* points, int stride, const int* counts, int fixed_count, int num_sets,
                  int minimum_good, double threshold, unsigned long long seed, RansacRecord* records, unsigned char* mask) {
  const size_t lds = static_cast<size_t>(stride) * sizeof(float4);
  if (!(ctx->func_attr_set & kFuncAttrFeatureRansac)) {
    DLIOM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(feature_ransac_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kMaxGood * static_cast<int>(sizeof(float4))));
    ctx->func_attr_set |= kFuncAttrFeatureRansac;
  }
  hipLaunchKernelGGL(feature_ransac_kernel, dim3(static_cast<unsigned>(num_sets)), dim3(kRansacThreads), lds, ctx->stream, points, stride,
                     counts, fixed_count, minimum_good, threshold * threshold, seed, records, mask);
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

// a stored set's key points from the records of dliom_surf_detect_and_compute: (x, y) of each
__global__ __launch_bounds__(256) void feature_keypoints_xy_kernel(const float* __restrict__ records, int n, float2* __restrict__ xy) {
  const int k = static_cast<int>(blockIdx.x) * 256 + threadIdx.x;
  if (k < n) xy[k] = make_float2(records[DLIOM_SURF_KEYPOINT_FLOATS * k], records[DLIOM_SURF_KEYPOINT_FLOATS * k + 1]);
}

bool all_finite(const float* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

void finish_model(double a, double b, double* scale, double* theta) {
  *scale = std::sqrt(a * a + b * b);
  *theta = std::atan2(b, a);
}

struct FeatureSet {
  float* descriptors = nullptr;  // HBM
  float* keypoints = nullptr;
  int count = 0;
  double ox = 0.0, oy = 0.0, resolution = 0.0;
};

}  // namespace
}  // namespace dliom

struct dliom_feature_index {
  dliom_ctx* ctx = nullptr;
  int D = 0;
  std::map<int64_t, dliom::FeatureSet> sets;
  int64_t keypoints = 0;
  dliom::DevBuf pairs, knn, points, small;  // the pair table; j0 j1 d0 d1; the good matches' points; counts and records
  int poll_us = 150;  // poll window of a match's completion word: twice what the previous match took (as the histogram's)
};

using dliom::FeaturePair;
using dliom::FeatureSet;
using dliom::RansacRecord;

extern "C" {

int dliom_feature_index_create(dliom_ctx* ctx, int descriptor_size, dliom_feature_index** index) {
  if (ctx == nullptr || index == nullptr || descriptor_size < 4 || descriptor_size > 128 || descriptor_size % 4 != 0)
    return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_feature_index* f = new dliom_feature_index();
  f->ctx = ctx;
  f->D = descriptor_size;
  *index = f;
  return DLIOM_OK;
}

void dliom_feature_index_destroy(dliom_feature_index* index) {
  if (index == nullptr) return;
  (void)hipSetDevice(index->ctx->device);
  (void)hipStreamSynchronize(index->ctx->stream);
  for (auto& e : index->sets) {
    if (e.second.descriptors != nullptr) (void)hipFree(e.second.descriptors);
    if (e.second.keypoints != nullptr) (void)hipFree(e.second.keypoints);
  }
  index->pairs.release();
  index->knn.release();
  index->points.release();
  index->small.release();
  delete index;
}

int dliom_feature_index_size(const dliom_feature_index* index, int64_t* num_sets) {
  if (index == nullptr || num_sets == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *num_sets = static_cast<int64_t>(index->sets.size());
  return DLIOM_OK;
}

int dliom_feature_index_memory_stats(const dliom_feature_index* index, dliom_feature_index_memory* out) {
  if (index == nullptr || out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  out->sets = static_cast<int64_t>(index->sets.size());
  out->keypoints = index->keypoints;
  out->descriptor_bytes = index->keypoints * index->D * static_cast<int64_t>(sizeof(float));
  out->keypoint_bytes = index->keypoints * 2 * static_cast<int64_t>(sizeof(float));
  out->scratch_bytes = static_cast<int64_t>(index->pairs.cap + index->knn.cap + index->points.cap + index->small.cap);
  return DLIOM_OK;
}

int dliom_feature_index_add(dliom_feature_index* index, int64_t key, const float* descriptors, const float* keypoints_xy,
                            int32_t count, double ox, double oy, double resolution) {
  if (index == nullptr || count < 0 || count > DLIOM_FEATURE_MAX_KEYPOINTS) return DLIOM_ERR_INVALID_ARGUMENT;
  if (count > 0 && (descriptors == nullptr || keypoints_xy == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(resolution)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (index->sets.count(key) != 0) return DLIOM_ERR_INVALID_ARGUMENT;
  const size_t n = static_cast<size_t>(count);
  if (!dliom::all_finite(descriptors, n * index->D) || !dliom::all_finite(keypoints_xy, n * 2)) return DLIOM_ERR_INVALID_ARGUMENT;
  FeatureSet s;
  s.count = count;
  s.ox = ox;
  s.oy = oy;
  s.resolution = resolution;
  if (count > 0) {
    dliom_ctx* ctx = index->ctx;
    DLIOM_HIP_TRY(hipSetDevice(ctx->device));
    DLIOM_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s.descriptors), n * index->D * sizeof(float)));
    if (hipMalloc(reinterpret_cast<void**>(&s.keypoints), n * 2 * sizeof(float)) != hipSuccess) {
      (void)hipFree(s.descriptors);
      return DLIOM_ERR_HIP;
    }
    hipError_t e = hipMemcpyAsync(s.descriptors, descriptors, n * index->D * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.keypoints, keypoints_xy, n * 2 * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller's arrays are consumed on return
    if (e != hipSuccess) {
      dliom::set_last_error("dliom_feature_index_add upload", e, __FILE__, __LINE__);
      (void)hipFree(s.descriptors);
      (void)hipFree(s.keypoints);
      return DLIOM_ERR_HIP;
    }
  }
  index->sets.emplace(key, s);
  index->keypoints += count;
  return DLIOM_OK;
}

int dliom_feature_index_add_from_grid(dliom_feature_index* index, int64_t key, const dliom_grid* grid,
                                      const double transform7[7], const dliom_surf_options* options, int32_t* count, double* ox,
                                      double* oy, double* resolution) {
  if (index == nullptr || grid == nullptr || transform7 == nullptr || grid->ctx != index->ctx ||
      index->D != DLIOM_SURF_DESCRIPTOR_SIZE || index->sets.count(key) != 0)
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_TRY(dliom::surf_check_options(options));
  dliom_ctx* ctx = index->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const uint8_t* image = nullptr;
  int32_t width = 0, height = 0;
  FeatureSet s;
  DLIOM_TRY(dliom::project_to_image_on_device(grid, transform7, &image, &width, &height, &s.ox, &s.oy, &s.resolution));
  const float *records = nullptr, *descriptors = nullptr;
  if (image != nullptr)
    DLIOM_TRY(dliom::surf_features_on_device(ctx, image, width, height, *options, &records, &descriptors, &s.count));
  if (s.count > 0) {
    const size_t n = static_cast<size_t>(s.count);
    DLIOM_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s.descriptors), n * index->D * sizeof(float)));
    if (hipMalloc(reinterpret_cast<void**>(&s.keypoints), n * 2 * sizeof(float)) != hipSuccess) {
      (void)hipFree(s.descriptors);
      return DLIOM_ERR_HIP;
    }
    hipError_t e = hipMemcpyAsync(s.descriptors, descriptors, n * index->D * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(dliom::feature_keypoints_xy_kernel, dim3(dliom::blocks_of(s.count, 256)), dim3(256), 0, ctx->stream, records,
                         s.count, reinterpret_cast<float2*>(s.keypoints));
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the scratch the set was copied from is free again
    if (e != hipSuccess) {
      dliom::set_last_error("dliom_feature_index_add_from_grid copy", e, __FILE__, __LINE__);
      (void)hipFree(s.descriptors);
      (void)hipFree(s.keypoints);
      return DLIOM_ERR_HIP;
    }
  }
  index->sets.emplace(key, s);
  index->keypoints += s.count;
  if (count != nullptr) *count = s.count;
  if (ox != nullptr) *ox = s.ox;
  if (oy != nullptr) *oy = s.oy;
  if (resolution != nullptr) *resolution = s.resolution;
  return DLIOM_OK;
}

int dliom_feature_index_remove(dliom_feature_index* index, int64_t key) {
  if (index == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  auto it = index->sets.find(key);
  if (it == index->sets.end()) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(index->ctx->device));
  DLIOM_HIP_TRY(hipStreamSynchronize(index->ctx->stream));
  if (it->second.descriptors != nullptr) (void)hipFree(it->second.descriptors);
  if (it->second.keypoints != nullptr) (void)hipFree(it->second.keypoints);
  index->keypoints -= it->second.count;
  index->sets.erase(it);
  return DLIOM_OK;
}

int dliom_feature_index_match(dliom_feature_index* index, int64_t query_key, const int64_t* train_keys, int count,
                              const dliom_feature_match_options* options, dliom_submap_match* results,
                              dliom_feature_match_stats* stats) {
  using namespace dliom;
  if (index == nullptr || options == nullptr || count < 0 || (count > 0 && (train_keys == nullptr || results == nullptr)))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(options->good_match_ratio_of_distance) || options->good_match_ratio_of_distance < 0.0 ||
      !std::isfinite(options->ransac_threshold) || options->ransac_threshold < 0.0 ||
      !std::isfinite(options->scale_estimated_tolerance) || options->scale_estimated_tolerance < 0.0 ||
      options->minimum_good_match_num < 0)
    return DLIOM_ERR_INVALID_ARGUMENT;
  const auto query_it = index->sets.find(query_key);
  if (query_it == index->sets.end()) return DLIOM_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < count; ++k)
    if (index->sets.count(train_keys[k]) == 0) return DLIOM_ERR_INVALID_ARGUMENT;
  if (count > DLIOM_FEATURE_MAX_TRAIN_SETS) return DLIOM_ERR_TOO_LARGE;
  dliom_feature_match_stats st = {};
  st.pairs = count;
  dliom_ctx* ctx = index->ctx;
  const FeatureSet& query = query_it->second;
  const int nq = query.count;
  // the pair table, in the page-locked block; a pair with a set of fewer than two key points never reaches the device
  FeaturePair* table = pinned_at<FeaturePair>(ctx, kPinFeaturePairs);
  int on_device = 0;
  for (int k = 0; k < count; ++k) {
    const FeatureSet& t = index->sets.find(train_keys[k])->second;
    const bool matched = nq >= 2 && t.count >= 2;
    table[k] = FeaturePair{t.descriptors, t.keypoints, matched ? t.count : 0, static_cast<float>(t.ox), static_cast<float>(t.oy), 0};
    on_device += matched ? 1 : 0;
    results[k] = dliom_submap_match{train_keys[k], DLIOM_FEATURE_TOO_FEW_KEYPOINTS, 0, 0, -1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  }
  if (on_device > 0) {
    DLIOM_HIP_TRY(hipSetDevice(ctx->device));
    const int stride = std::min(nq, kMaxGood);
    const size_t per_array = align256(static_cast<size_t>(count) * nq * sizeof(float));
    DLIOM_TRY(index->pairs.reserve(static_cast<size_t>(count) * sizeof(FeaturePair)));
    DLIOM_TRY(index->knn.reserve(4 * per_array));
    DLIOM_TRY(index->points.reserve(static_cast<size_t>(count) * stride * sizeof(float4)));
    const size_t counts_bytes = align256(static_cast<size_t>(count) * sizeof(int));
    DLIOM_TRY(index->small.reserve(counts_bytes + static_cast<size_t>(count) * sizeof(RansacRecord)));
    char* const knn = index->knn.as<char>();
    int* const j0 = reinterpret_cast<int*>(knn);
    int* const j1 = reinterpret_cast<int*>(knn + per_array);
    float* const d0 = reinterpret_cast<float*>(knn + 2 * per_array);
    float* const d1 = reinterpret_cast<float*>(knn + 3 * per_array);
    int* const counts = index->small.as<int>();
    RansacRecord* const records = reinterpret_cast<RansacRecord*>(index->small.as<char>() + counts_bytes);
    const bool timed = ctx->profiling && stats != nullptr;
    struct Events {  // destroyed on every way out
      hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
      ~Events() {
        for (hipEvent_t x : e)
          if (x != nullptr) (void)hipEventDestroy(x);
      }
    } events;
    hipEvent_t* const ev = events.e;
    if (timed)
      for (hipEvent_t& e : events.e) DLIOM_HIP_TRY(hipEventCreate(&e));
    const auto enqueued_at = std::chrono::steady_clock::now();
    DLIOM_HIP_TRY(hipMemcpyAsync(index->pairs.p, table, static_cast<size_t>(count) * sizeof(FeaturePair), hipMemcpyHostToDevice,
                                 ctx->stream));
    const FeaturePair* pairs = index->pairs.as<FeaturePair>();
    if (timed) DLIOM_HIP_TRY(hipEventRecord(ev[0], ctx->stream));
    DLIOM_TRY(launch_knn(ctx->stream, index->D, query.descriptors, nq, pairs, count, j0, j1, d0, d1));
    if (timed) DLIOM_HIP_TRY(hipEventRecord(ev[1], ctx->stream));
    hipLaunchKernelGGL(feature_good_kernel, dim3(static_cast<unsigned>(count)), dim3(256), 0, ctx->stream, query.keypoints, nq,
                       static_cast<float>(query.ox), static_cast<float>(query.oy), query.resolution,
                       options->good_match_ratio_of_distance, pairs, j0, d0, d1, index->points.as<float4>(), stride, counts);
    DLIOM_HIP_TRY(hipGetLastError());
    if (timed) DLIOM_HIP_TRY(hipEventRecord(ev[2], ctx->stream));
    DLIOM_TRY(launch_ransac(ctx, index->points.as<float4>(), stride, counts, 0, count, options->minimum_good_match_num,
                            options->ransac_threshold, options->seed, records, nullptr));
    if (timed) DLIOM_HIP_TRY(hipEventRecord(ev[3], ctx->stream));
    RansacRecord* const host = pinned_at<RansacRecord>(ctx, kPinFeatureResults);
    const unsigned words = static_cast<unsigned>(static_cast<size_t>(count) * sizeof(RansacRecord) / 4);
    if (ctx->done_word != nullptr) {
      const unsigned seq = next_done_seq(ctx);
      hipLaunchKernelGGL(feature_readback_kernel, dim3(1), dim3(1024), 0, ctx->stream, reinterpret_cast<const unsigned*>(records),
                         words, reinterpret_cast<unsigned*>(host), ctx->done_word, seq);
      DLIOM_HIP_TRY(hipGetLastError());
      DLIOM_TRY(wait_done(ctx, ctx->stream, ctx->done_word, seq, index->poll_us));
      const auto took = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - enqueued_at).count();
      index->poll_us = static_cast<int>(std::min<long long>(std::max<long long>(2 * took, 150), 100000));
    } else {
      hipLaunchKernelGGL(feature_readback_kernel, dim3(1), dim3(1024), 0, ctx->stream, reinterpret_cast<const unsigned*>(records),
                         words, reinterpret_cast<unsigned*>(host), static_cast<unsigned*>(nullptr), 0u);
      DLIOM_HIP_TRY(hipGetLastError());
      DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    st.read_backs = 1;
    if (timed) {
      DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
      float ms[3] = {0.f, 0.f, 0.f};
      for (int k = 0; k < 3; ++k) DLIOM_HIP_TRY(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
      st.knn_ms = ms[0];
      st.good_ms = ms[1];
      st.ransac_ms = ms[2];
    }
    for (int k = 0; k < count; ++k) {
      if (table[k].nt < 2) continue;
      const RansacRecord& r = host[k];
      dliom_submap_match& out = results[k];
      out.good_matches = r.good;
      if (r.flags & kFlagCapacity) {
        out.status = DLIOM_ERR_CAPACITY;
      } else if (!(r.flags & kFlagEvaluated)) {
        out.status = DLIOM_FEATURE_TOO_FEW_GOOD_MATCHES;
      } else if (r.flags & kFlagNoModel) {
        out.status = DLIOM_FEATURE_NO_MODEL;
      } else {
        out.inliers = r.inliers;
        out.hypothesis = r.hypothesis;
        out.a = r.a;
        out.b = r.b;
        out.tx = r.tx;
        out.ty = r.ty;
        finish_model(r.a, r.b, &out.scale, &out.theta);
        out.status = std::abs(out.scale - 1.0) > options->scale_estimated_tolerance ? DLIOM_FEATURE_SCALE_REJECTED : DLIOM_FEATURE_MATCHED;
      }
      st.ransac_pairs += (r.flags & kFlagEvaluated) ? 1 : 0;
    }
  }
  for (int k = 0; k < count; ++k) {
    switch (results[k].status) {
      case DLIOM_FEATURE_MATCHED: ++st.matched; break;
      case DLIOM_FEATURE_TOO_FEW_KEYPOINTS: ++st.too_few_keypoints; break;
      case DLIOM_FEATURE_TOO_FEW_GOOD_MATCHES: ++st.too_few_good_matches; break;
      case DLIOM_FEATURE_NO_MODEL: ++st.no_model; break;
      case DLIOM_FEATURE_SCALE_REJECTED: ++st.scale_rejected; break;
      default: ++st.over_capacity; break;
    }
  }
  if (stats != nullptr) *stats = st;
  return DLIOM_OK;
}

int dliom_feature_index_knn(dliom_feature_index* index, int64_t query_key, int64_t train_key, int32_t* j0, int32_t* j1,
                            float* d0, float* d1) {
  using namespace dliom;
  if (index == nullptr || j0 == nullptr || j1 == nullptr || d0 == nullptr || d1 == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  const auto q = index->sets.find(query_key), t = index->sets.find(train_key);
  if (q == index->sets.end() || t == index->sets.end() || q->second.count < 2 || t->second.count < 2)
    return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_ctx* ctx = index->ctx;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const int nq = q->second.count;
  const size_t per_array = align256(static_cast<size_t>(nq) * sizeof(float));
  DLIOM_TRY(index->pairs.reserve(sizeof(FeaturePair)));
  DLIOM_TRY(index->knn.reserve(4 * per_array));
  const FeaturePair pair{t->second.descriptors, t->second.keypoints, t->second.count, static_cast<float>(t->second.ox),
                         static_cast<float>(t->second.oy), 0};
  DLIOM_HIP_TRY(hipMemcpyAsync(index->pairs.p, &pair, sizeof(pair), hipMemcpyHostToDevice, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // `pair` is on this frame
  char* const knn = index->knn.as<char>();
  DLIOM_TRY(launch_knn(ctx->stream, index->D, q->second.descriptors, nq, index->pairs.as<FeaturePair>(), 1,
                       reinterpret_cast<int*>(knn), reinterpret_cast<int*>(knn + per_array),
                       reinterpret_cast<float*>(knn + 2 * per_array), reinterpret_cast<float*>(knn + 3 * per_array)));
  void* const host[4] = {j0, j1, d0, d1};
  for (int k = 0; k < 4; ++k)
    DLIOM_HIP_TRY(hipMemcpyAsync(host[k], knn + k * per_array, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DLIOM_OK;
}

int dliom_feature_ransac(dliom_ctx* ctx, const float* from_xy, const float* to_xy, int num_matches, double threshold,
                         uint64_t seed, dliom_feature_ransac_result* result, unsigned char* inlier_mask) {
  using namespace dliom;
  if (ctx == nullptr || from_xy == nullptr || to_xy == nullptr || result == nullptr || num_matches < 2 ||
      num_matches > kMaxGood || !std::isfinite(threshold) || threshold < 0.0)
    return DLIOM_ERR_INVALID_ARGUMENT;
  const size_t M = static_cast<size_t>(num_matches);
  if (!all_finite(from_xy, 2 * M) || !all_finite(to_xy, 2 * M)) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  std::vector<float> packed(4 * M);
  for (size_t k = 0; k < M; ++k) {
    packed[4 * k] = from_xy[2 * k];
    packed[4 * k + 1] = from_xy[2 * k + 1];
    packed[4 * k + 2] = to_xy[2 * k];
    packed[4 * k + 3] = to_xy[2 * k + 1];
  }
  const size_t points_bytes = align256(M * sizeof(float4)), record_bytes = align256(sizeof(RansacRecord));
  DLIOM_TRY(ctx->misc.reserve(points_bytes + record_bytes + align256(M)));
  char* const base = ctx->misc.as<char>();
  RansacRecord* const record = reinterpret_cast<RansacRecord*>(base + points_bytes);
  unsigned char* const mask = reinterpret_cast<unsigned char*>(base + points_bytes + record_bytes);
  DLIOM_HIP_TRY(hipMemcpyAsync(base, packed.data(), M * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  DLIOM_TRY(launch_ransac(ctx, reinterpret_cast<const float4*>(base), num_matches, nullptr, num_matches, 1, 0, threshold,
                          seed, record, mask));
  RansacRecord r;
  std::vector<unsigned char> m(M);
  DLIOM_HIP_TRY(hipMemcpyAsync(&r, record, sizeof(r), hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipMemcpyAsync(m.data(), mask, M, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const int all_pairs = num_matches * (num_matches - 1) / 2;
  *result = dliom_feature_ransac_result{DLIOM_FEATURE_NO_MODEL, 0, -1,
                                        std::min(all_pairs, DLIOM_FEATURE_RANSAC_HYPOTHESES), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (!(r.flags & kFlagNoModel)) {
    result->status = DLIOM_FEATURE_MATCHED;
    result->inliers = r.inliers;
    result->hypothesis = r.hypothesis;
    result->a = r.a;
    result->b = r.b;
    result->tx = r.tx;
    result->ty = r.ty;
    finish_model(r.a, r.b, &result->scale, &result->theta);
  }
  if (inlier_mask != nullptr) std::memcpy(inlier_mask, m.data(), M);
  return DLIOM_OK;
}

}  // extern "C"
