// The exact 3-D nearest-neighbour index (nn_index.hip) as icp.hip sees it: dliom.h "scan alignment by ICP".
#ifndef DLIOM_CSRC_NN_INDEX_H_
#define DLIOM_CSRC_NN_INDEX_H_

#include "internal.h"

namespace dliom {

constexpr int kNnShells = DLIOM_NN_MAX_SHELLS;

// Device view of an index, passed by value to the kernels.
struct NnGridView {
  const float4* sorted;   // the finite target points by cell: x, y, z and the point's index in the cloud (as bits)
  const float4* by_index; // every target point in the cloud's order: x, y, z (what a correspondence's sums read)
  const int* cell_start;  // cells + 1 entries: cell c holds sorted[cell_start[c] .. cell_start[c + 1])
  int n_finite;
  int dims[3];
  float lo[3], hi[3];     // the finite points' bounding box
  float inv;              // cells a metre
  double edge;            // 1 / inv, rounded once (0 under the one-cell grid): the stop rule of nn_shell_kernel
};

// Words of an index's counter block
enum : int { kNnListCount = 0, kNnByGrid = 1, kNnByBruteForce = 2, kNnNonFinite = 3, kNnCounterWords = 4 };

// p = (float)(((r00*x + r01*y) + r02*z) + t0) ... in double from float points, m: 12 doubles (3 rows of r0 r1 r2 t);
// in place is fine.
struct Rigid12 {
  double m[12];
};
int nn_transform_enqueue(dliom_ctx* ctx, const float* x, const float* y, const float* z, int n, const Rigid12& m, float* ox,
                         float* oy, float* oz);

// One search, only enqueued on the context's stream.  px/py/pz: n query points in HBM; j (-1: none) and d2 (+inf: none):
// n entries each; key: n 64-bit words and list: n ints of scratch; counters: kNnCounterWords ints of which [kNnListCount]
// is zero on entry.  The caller zeroes [kNnListCount] behind the search.
struct NnSearch {
  const float *px, *py, *pz;
  int n;
  int* j;
  float* d2;
  unsigned long long* key;  // 8-byte aligned
  int* list;
  int* counters;
};
int nn_search_enqueue(dliom_nn_index* index, const NnSearch& s, double max_distance_squared, int search);
NnGridView nn_view(const dliom_nn_index* index);
dliom_ctx* nn_ctx(const dliom_nn_index* index);
DevBuf* nn_scratch(dliom_nn_index* index);  // grow-only, free between the index's calls
int* nn_poll_us(dliom_nn_index* index);

// ---- many searches in one launch chain (icp_batch.hip): a table of items in HBM, `stride` bytes apart, one per pair on
// the list.  The pair is a grid dimension of the batched kernels, which run the single kernels' bodies with the item's
// view, search and bound: the same (j, d2) bits and the same counters as nn_search_enqueue gives that pair alone.
struct NnBatchItem {
  NnGridView view;
  NnSearch search;         // counters: the pair's own block
  double max_d2;
  int brute;               // every query by the brute-force scan (nn_batch_item: the option and the index's own mode)
  int segments, segment;   // of the brute-force scan over this pair's target (nn_batch_item)
  int transform;           // nn_transform_batch_enqueue: 0 nothing; else (ox, oy, oz) <- (float)(m * (sx, sy, sz)), in place is fine
  const float *sx, *sy, *sz;
  float *ox, *oy, *oz;     // search.px, py, pz as the transform writes them
  Rigid12 m;
};
// view, brute, segments and segment of a search on `index` under the option `search` (DLIOM_NN_*)
void nn_batch_item(const dliom_nn_index* index, int search, NnBatchItem* item);
// count items from `table` (device); max_n: the largest search.n among them, max_segments likewise.  Only enqueued.
int nn_batch_pairs_per_launch(int max_n);  // a launch holds at most 2^30 lanes: the pairs of a table go in runs of this many
int nn_transform_batch_enqueue(dliom_ctx* ctx, const void* table, size_t stride, int count, int max_n);
int nn_search_batch_enqueue(dliom_ctx* ctx, const void* table, size_t stride, int count, int max_n, int max_segments);

// icp.hip: dliom.h's fitness score of n points in HBM (n <= DLIOM_NN_MAX_POINTS) against the index's target: the mean of
// d2 without a bound by the fixed tree (NaN when *count is 0); one polled read-back
int icp_fitness_of(dliom_nn_index* index, const float* x, const float* y, const float* z, int n, double* score, long long* count);

}  // namespace dliom

#endif  // DLIOM_CSRC_NN_INDEX_H_
