// The fixed tree of dliom.h "scan alignment by ICP" (DLIOM_ICP_TREE_MIN_LEAVES), stated once for its callers (icp.hip: 16
// sums over the correspondences; ndt.hip: 7, 21 or 28 sums over the per-point values): S double sums and an int count over
// the leaf index, +0.0 beyond the last leaf, adjacent pairs added level by level -- a function of the index alone.
//   tree_reduce_kernel<S, Leaves>  one workgroup per 2048 consecutive leaves: a lane sums 8 adjacent leaves pairwise, the
//                                  workgroup its 256 lanes pairwise through LDS -- the subtree over those 2048 leaves
//                                  (tree_reduce_block, the body, is also what a batched reduction runs per pair)
//   tree_finish<S>                 inside a one-workgroup kernel: the tree over the workgroups' partial sums, padded with
//                                  +0.0 to a power of two; the root is left in partials[0 .. S)
// Leaves: a struct passed by value with  __device__ void leaf(int i, double v[S], int* count) const  (all +0.0 and 0 for
// an i at or beyond its length).
#ifndef DLIOM_CSRC_TREE_REDUCE_H_
#define DLIOM_CSRC_TREE_REDUCE_H_

#include "internal.h"

namespace dliom {

constexpr int kTreeThreads = 256;
constexpr int kTreeLeavesPerLane = 8;
constexpr int kTreeLeavesPerBlock = kTreeThreads * kTreeLeavesPerLane;
static_assert(kTreeLeavesPerBlock == DLIOM_ICP_TREE_MIN_LEAVES, "the tree's least size is one workgroup's subtree");

// The subtree over the W leaves from `first` (W a power of two): left half + right half
template <int S, int W, class Leaves>
__device__ __forceinline__ void tree_subtree(const Leaves& L, int first, double v[S], int* count) {
  if constexpr (W == 1) {
    L.leaf(first, v, count);
  } else {
    double r[S];
    int c = 0;
    tree_subtree<S, W / 2>(L, first, v, count);
    tree_subtree<S, W / 2>(L, first + W / 2, r, &c);
    for (int k = 0; k < S; ++k) v[k] = v[k] + r[k];
    *count += c;
  }
}

// One workgroup's subtree: the 2048 leaves from block * 2048, into partials[block * S ..) and counts[block].  Called by every
// lane of a kTreeThreads workgroup (tree_reduce_kernel; icp_batch.hip's and ndt_batch.hip's kernels, where the block is one of a pair's)
template <int S, class Leaves>
__device__ __forceinline__ void tree_reduce_block(const Leaves& L, int block, double* __restrict__ partials, int* __restrict__ counts) {
  __shared__ double lds[kTreeThreads * S];
  __shared__ int lds_count[kTreeThreads];
  double v[S];
  int count = 0;
  tree_subtree<S, kTreeLeavesPerLane>(L, (block * kTreeThreads + static_cast<int>(threadIdx.x)) * kTreeLeavesPerLane, v, &count);
  for (int k = 0; k < S; ++k) lds[threadIdx.x * S + k] = v[k];
  lds_count[threadIdx.x] = count;
  for (int w = 1; w < kTreeThreads; w <<= 1) {  // adjacent pairs, level by level
    __syncthreads();
    const int pairs = kTreeThreads / (2 * w);
    for (int e = threadIdx.x; e < pairs * S; e += kTreeThreads) {
      const int left = (e / S) * 2 * w, k = e % S;
      lds[left * S + k] = lds[left * S + k] + lds[(left + w) * S + k];
    }
    if (static_cast<int>(threadIdx.x) < pairs) lds_count[threadIdx.x * 2 * w] += lds_count[threadIdx.x * 2 * w + w];
  }
  __syncthreads();
  if (threadIdx.x < S) partials[static_cast<size_t>(block) * S + threadIdx.x] = lds[threadIdx.x];
  if (threadIdx.x == 0) counts[block] = lds_count[0];
}

template <int S, class Leaves>
__global__ __launch_bounds__(kTreeThreads) void tree_reduce_kernel(Leaves L, double* __restrict__ partials, int* __restrict__ counts) {
  tree_reduce_block<S, Leaves>(L, static_cast<int>(blockIdx.x), partials, counts);
}

// partials: room for P2 >= P entries of S, P2 a power of two; called by every lane of a kTreeThreads workgroup
template <int S>
__device__ __forceinline__ void tree_finish(double* partials, int P, int P2) {
  for (int e = P * S + threadIdx.x; e < P2 * S; e += kTreeThreads) partials[e] = 0.0;
  for (int w = 1; w < P2; w <<= 1) {
    __syncthreads();
    const int pairs = P2 / (2 * w);
    for (int e = threadIdx.x; e < pairs * S; e += kTreeThreads) {
      const size_t left = static_cast<size_t>(e / S) * 2 * w;
      const int k = e % S;
      partials[left * S + k] = partials[left * S + k] + partials[(left + w) * S + k];
    }
  }
  __syncthreads();
}

// workgroups of the reduction over n leaves and the power of two that holds them
inline void tree_geometry(int n, int* P, int* P2) {
  *P = static_cast<int>(blocks_of(n > 1 ? n : 1, kTreeLeavesPerBlock));
  *P2 = 1;
  while (*P2 < *P) *P2 <<= 1;
}

}  // namespace dliom

#endif  // DLIOM_CSRC_TREE_REDUCE_H_
