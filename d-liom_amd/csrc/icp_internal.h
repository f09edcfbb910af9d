// What an alignment of one pair (icp.hip) and of many pairs in lock step (icp_batch.hip) share: the leaves of the sixteen
// sums, the read-back of one iteration and the kernel body that writes it, and the host's solve, composition, checks and
// decision (defined in icp.hip).  Stated once, so that a pair gets the same bits whichever call aligns it.
#ifndef DLIOM_CSRC_ICP_INTERNAL_H_
#define DLIOM_CSRC_ICP_INTERNAL_H_

#include "device_common.h"
#include "nn_index.h"
#include "tree_reduce.h"

namespace dliom {

constexpr int kIcpSums = 16;  // Sp (3), Sq (3), Spq (9, row-major), Sd

struct IcpLeaves {
  const float *px, *py, *pz;
  const int* j;
  const float* d2;
  const float4* by_index;
  int n;
  __device__ __forceinline__ void leaf(int i, double v[kIcpSums], int* count) const {
    const bool has = i < n && j[i] >= 0;
    if (has) {
      const double p[3] = {px[i], py[i], pz[i]};
      const float4 t = by_index[j[i]];
      const double q[3] = {t.x, t.y, t.z};
      for (int a = 0; a < 3; ++a) {
        v[a] = p[a];
        v[3 + a] = q[a];
        for (int b = 0; b < 3; ++b) v[6 + 3 * a + b] = p[a] * q[b];
      }
      v[15] = static_cast<double>(d2[i]);
    } else {
      for (int k = 0; k < kIcpSums; ++k) v[k] = 0.0;
    }
    *count = has ? 1 : 0;
  }
};

struct IcpReadback {  // kPinIcpSums; a slot of kPinIcpBatchReadback
  double sums[kIcpSums];
  long long n;
  int counters[kNnCounterWords];
  unsigned max_sq, pad;
};
static_assert(sizeof(IcpReadback) == kPinIcpBatchSlotBytes && kPinIcpBatchPairs == DLIOM_ICP_BATCH_MAX_PAIRS,
              "pinned_layout.h's slots are read-backs, one for each pair in flight");

// Called by every lane of a kTreeThreads workgroup: the tree over the P partial sums of one search (partials: room for P2 >= P
// entries, P2 a power of two), then the sums, the count and the search's counters into *out (page-locked).  The caller
// makes them visible to the host.
__device__ __forceinline__ void icp_finish_body(double* partials, const int* __restrict__ counts, int P, int P2, int* counters,
                                                const unsigned* max_sq, IcpReadback* out) {
  tree_finish<kIcpSums>(partials, P, P2);
  if (threadIdx.x < kIcpSums) out->sums[threadIdx.x] = partials[threadIdx.x];
  if (threadIdx.x == 0) {
    long long n = 0;
    for (int b = 0; b < P; ++b) n += counts[b];
    out->n = n;
    for (int k = 0; k < kNnCounterWords; ++k) out->counters[k] = counters[k];
    counters[kNnListCount] = 0;  // the next search's list starts empty
    out->max_sq = max_sq != nullptr ? *max_sq : 0u;
  }
}

// ---- many pairs in lock step (icp_batch.hip; the final rounds of ndt_batch.hip): a pair's descriptor in the round's table
// and the bodies of the kernels that take the pair as a grid dimension.  A workgroup outside its pair's extent leaves as
// a whole before any barrier.
struct IcpBatchEntry {
  NnBatchItem nn;
  double* partials;
  int* counts;
  int P, P2;
  unsigned* max_sq;
  int want_norm;  // this is the pair's fitness step and its cloud is wanted
  int slot;       // of the round's read-back slots
};

__device__ __forceinline__ const IcpBatchEntry& icp_batch_entry(const char* table, size_t stride, unsigned pair) {
  return *reinterpret_cast<const IcpBatchEntry*>(table + stride * pair);
}

__device__ __forceinline__ void icp_batch_max_norm_body(const IcpBatchEntry& d, int block) {
  const int n = d.nn.search.n;
  if (d.want_norm == 0 || block * kTreeThreads >= n) return;
  const int i = block * kTreeThreads + static_cast<int>(threadIdx.x);
  note_kept(i < n ? norm_word(d.nn.search.px[i], d.nn.search.py[i], d.nn.search.pz[i]) : 0u, d.max_sq);
}

__device__ __forceinline__ void icp_batch_reduce_body(const IcpBatchEntry& d, int block) {
  if (block >= d.P) return;
  const IcpLeaves L{d.nn.search.px, d.nn.search.py, d.nn.search.pz, d.nn.search.j, d.nn.search.d2, d.nn.view.by_index, d.nn.search.n};
  tree_reduce_block<kIcpSums, IcpLeaves>(L, block, d.partials, d.counts);
}

// a workgroup a pair: tree_finish over that pair's partial sums, into the pair's read-back slot (page-locked)
__device__ __forceinline__ void icp_batch_finish_body(const IcpBatchEntry& d, IcpReadback* out) {
  icp_finish_body(d.partials, d.counts, d.P, d.P2, d.nn.search.counters, d.max_sq, out);
  __threadfence_system();  // the slot is in the host's memory before this workgroup ends
}

// one completion word behind everything on the stream
__device__ __forceinline__ void batch_done_body(unsigned* done_word, unsigned done_seq) {
  if (threadIdx.x == 0) {
    __threadfence_system();
    *reinterpret_cast<volatile unsigned*>(done_word) = done_seq;
  }
}

// icp.hip
void icp_solve(const double S[kIcpSums], long long n, double R[9], double t[3]);
void icp_compose(const double R[9], const double t[3], double T[16]);  // T <- [R t; 0 0 0 1] T
Rigid12 rigid_of(const double R[9], const double t[3]);
bool icp_options_ok(const dliom_icp_options* o);
bool icp_guess_ok(const double* g);
bool icp_iterate(const dliom_icp_options* options, const double sums[kIcpSums], long long n, int k, double* previous_mse,
                 dliom_icp_result* res, double R[9], double t[3], bool* ends);
// bytes of an alignment's device arrays for n source points, without the 256 bytes of counters in front (icp_carve;
// dliom_icp_batch_scratch_bytes)
size_t icp_work_bytes(int64_t n);

}  // namespace dliom

#endif  // DLIOM_CSRC_ICP_INTERNAL_H_
