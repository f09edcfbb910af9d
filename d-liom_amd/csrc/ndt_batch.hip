// Many scan pairs aligned by NDT in one call (dliom.h "scan alignment by NDT", dliom_ndt_align_batch): the `--method ndt`
// half of the loop of gen_ground_truth_by_ndt_match.cc:151-261.  The pairs of a chunk advance in lock step.  A round on the
// ACTIVE LIST -- the chunk's pairs that are not finished -- is one launch chain on the context's stream, with the pair as
// a grid dimension of every kernel.  The round's table holds, in this order, the pairs that evaluate everything, those
// that evaluate without the Hessian, those that evaluate the Hessian alone, then the pairs in their FINAL ROUND (their
// alignment is done; the fitness score and the aligned cloud are left), first those with a fitness index:
//   the upload            the pairs' descriptors (NdtBatchEval or NdtBatchFinal) from the page-locked table into HBM: one copy
//   ndt_batch_eval_kernel<G, H>  at most three launches, one per kind of evaluation on the list: ndt_eval_kernel's body
//   ndt_batch_reduce_kernel<S>   likewise: tree_reduce_kernel's tree, a workgroup per 2048 consecutive source indices of a pair
//   ndt_batch_finish_kernel      a workgroup a pair: tree_finish over that pair's partial sums, into that pair's read-back slot
//   nn_transform_batch_kernel (nn_index.hip)  the final points of the pairs in their final round
//   ndt_batch_max_norm_kernel    their norm bound, when the clouds are wanted
//   nn_shell / nn_brute / nn_resolve_batch_kernel (nn_index.hip)  the fitness search of those with an index
//   ndt_batch_fitness_reduce_kernel, ndt_batch_final_finish_kernel  ICP's sums and read-back (icp_internal.h's bodies)
//   ndt_batch_done_kernel        one completion word behind everything; the host polls it once (wait_done)
// Every kernel runs the body that the single call's kernel runs (ndt_internal.h, tree_reduce.h, nn_index.hip,
// icp_internal.h) and the host decides with the single call's state machine (NdtAlignment), one per pair, so a pair's
// result has the single call's bits.  A workgroup outside its pair's extent leaves as a whole before any barrier.  No
// floating-point atomics; the integer atomics (search counters, norm word) are each pair's own.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "icp_internal.h"
#include "ndt_internal.h"

namespace dliom {
namespace {

constexpr int kThreads = kTreeThreads;
static_assert(kNdtThreads == kTreeThreads, "one workgroup size for the whole chain");
constexpr size_t kEntryBytes = kPinNdtBatchEntryBytes;
constexpr size_t kSlotBytes = kPinNdtBatchSlotBytes;
// what dliom_ndt_batch_scratch_bytes counts in front of a pair's arrays: its descriptor and its counters
constexpr size_t kCounterBytes = 256;

// A pair that evaluates in this round
struct NdtBatchEval {
  NdtTable table;
  NdtPose pose;
  const float *sx, *sy, *sz;
  double* leaves;
  int* pairs;
  double* partials;
  int* counts;
  int n, P, P2;
  int what;  // DLIOM_NDT_EVAL_*
};
// A pair in its final round
struct NdtBatchFinal {
  IcpBatchEntry icp;  // nn.transform: the final points from the source; want_norm: the cloud is wanted
  int searched;       // it has a fitness index: the search and ICP's sums run
};
static_assert(sizeof(NdtBatchEval) <= kEntryBytes && sizeof(NdtBatchFinal) <= kEntryBytes && kEntryBytes % 8 == 0,
              "a descriptor fits its place");
static_assert(sizeof(IcpReadback) <= kSlotBytes && sizeof(NdtReadback) <= kSlotBytes && kSlotBytes % 8 == 0, "a read-back fits its slot");
static_assert(kPinNdtBatchPairs == DLIOM_NDT_BATCH_MAX_PAIRS, "pinned_layout.h has a slot and a descriptor for each pair in flight");

__device__ __forceinline__ const NdtBatchEval& eval_of(const char* table, unsigned pair) {
  return *reinterpret_cast<const NdtBatchEval*>(table + kEntryBytes * pair);
}
__device__ __forceinline__ const NdtBatchFinal& final_of(const char* table, unsigned pair) {
  return *reinterpret_cast<const NdtBatchFinal*>(table + kEntryBytes * pair);
}

// table: the first descriptor of this kind's run; the descriptor is uniform over the workgroup
template <bool G, bool H>
__global__ __launch_bounds__(kThreads) void ndt_batch_eval_kernel(const char* __restrict__ table) {
  const NdtBatchEval& d = eval_of(table, blockIdx.y);
  const int block = static_cast<int>(blockIdx.x);
  if (block * kThreads >= d.n) return;
  ndt_eval_body<G, H>(d.table, d.pose, d.sx, d.sy, d.sz, d.n, d.leaves, d.pairs, block);
}

template <int S>
__global__ __launch_bounds__(kThreads) void ndt_batch_reduce_kernel(const char* __restrict__ table) {
  const NdtBatchEval& d = eval_of(table, blockIdx.y);
  const int block = static_cast<int>(blockIdx.x);
  if (block >= d.P) return;
  const NdtLeaves<S> L{d.leaves, d.pairs, d.n};
  tree_reduce_block<S, NdtLeaves<S>>(L, block, d.partials, d.counts);
}

// table: the round's first descriptor (a pair's slot is its place in the table); the evaluating pairs of every kind
__global__ __launch_bounds__(kThreads) void ndt_batch_finish_kernel(const char* __restrict__ table, char* slots) {
  const NdtBatchEval& d = eval_of(table, blockIdx.x);
  NdtReadback* const out = reinterpret_cast<NdtReadback*>(slots + kSlotBytes * blockIdx.x);
  if (d.what == DLIOM_NDT_EVAL_GRADIENT)
    ndt_finish_body<ndt_sums(true, false)>(d.partials, d.counts, d.P, d.P2, out);
  else if (d.what == DLIOM_NDT_EVAL_ALL)
    ndt_finish_body<ndt_sums(true, true)>(d.partials, d.counts, d.P, d.P2, out);
  else
    ndt_finish_body<ndt_sums(false, true)>(d.partials, d.counts, d.P, d.P2, out);
  __threadfence_system();  // the slot is in the host's memory before this workgroup ends
}

// table: the first descriptor of the final rounds
__global__ __launch_bounds__(kThreads) void ndt_batch_max_norm_kernel(const char* __restrict__ table) {
  icp_batch_max_norm_body(final_of(table, blockIdx.y).icp, static_cast<int>(blockIdx.x));
}

__global__ __launch_bounds__(kThreads) void ndt_batch_fitness_reduce_kernel(const char* __restrict__ table) {
  icp_batch_reduce_body(final_of(table, blockIdx.y).icp, static_cast<int>(blockIdx.x));
}

// slots: the slot of the first final round.  A pair without a search leaves its norm bound and a count of 0.
__global__ __launch_bounds__(kThreads) void ndt_batch_final_finish_kernel(const char* __restrict__ table, char* slots) {
  const NdtBatchFinal& d = final_of(table, blockIdx.x);
  IcpReadback* const out = reinterpret_cast<IcpReadback*>(slots + kSlotBytes * blockIdx.x);
  if (d.searched != 0) {
    icp_batch_finish_body(d.icp, out);
    return;
  }
  if (threadIdx.x == 0) {
    out->n = 0;
    out->max_sq = *d.icp.max_sq;
  }
  __threadfence_system();
}

__global__ void ndt_batch_done_kernel(unsigned* done_word, unsigned done_seq) { batch_done_body(done_word, done_seq); }

struct Carve {  // a pair's arrays behind its descriptor and counters, in this order
  size_t leaves, pairs, partials, counts, icp, total;
  int P, P2;
};
Carve carve_of(int64_t n) {
  Carve c;
  tree_geometry(static_cast<int>(n), &c.P, &c.P2);
  const size_t m = static_cast<size_t>(std::max<int64_t>(n, 1));
  c.leaves = 0;
  c.pairs = c.leaves + align256(28 * m * sizeof(double));
  c.partials = c.pairs + align256(4 * m);
  c.counts = c.partials + align256(static_cast<size_t>(c.P2) * 28 * sizeof(double));
  c.icp = c.counts + align256(4 * static_cast<size_t>(c.P2));
  c.total = c.icp + icp_work_bytes(n);
  return c;
}
size_t pair_scratch_bytes(int64_t n) { return kEntryBytes + kCounterBytes + carve_of(n).total; }

// A pair of the chunk in flight
struct Pair {
  const dliom_ndt_pair* in = nullptr;
  int n = 0;
  dliom_ndt_result res = {};
  NdtAlignment machine;
  NdtRequest request;   // its next evaluation, while !aligned
  NdtSums sums;
  bool aligned = false; // the alignment is done: its next round is its final one
  NdtBatchEval eval;    // table, arrays, geometry; pose and what are set a round
  NdtBatchFinal last;
};

struct Events {  // four a round while profiling is on: upload and evaluations | reductions | the final rounds' chain
  dliom_ctx* ctx;
  bool timed;
  std::vector<hipEvent_t> e;
  ~Events() {
    for (hipEvent_t x : e) (void)hipEventDestroy(x);
  }
  int mark() {
    if (!timed) return DLIOM_OK;
    hipEvent_t x = nullptr;
    DLIOM_HIP_TRY(hipEventCreate(&x));
    e.push_back(x);
    DLIOM_HIP_TRY(hipEventRecord(x, ctx->stream));
    return DLIOM_OK;
  }
};

struct Batch {
  dliom_ctx* ctx;
  const dliom_ndt_options* options;
  dliom_ndt_batch_stats* stats;
  Events* events;
  int poll_us = 150;  // of the round's completion word: twice what the previous round took
  double host_ms = 0.0;
};

template <bool G, bool H>
int launch_kind(dliom_ctx* ctx, const char* table, int count, int max_n, int max_P, bool reduce) {
  constexpr int S = ndt_sums(G, H);
  const int run = nn_batch_pairs_per_launch(std::max(max_n, 1));
  for (int first = 0; first < count; first += run) {
    const unsigned pairs = static_cast<unsigned>(std::min(run, count - first));
    const char* const t = table + kEntryBytes * static_cast<size_t>(first);
    if (!reduce)
      hipLaunchKernelGGL((ndt_batch_eval_kernel<G, H>), dim3(blocks_of(max_n, kThreads), pairs), dim3(kThreads), 0, ctx->stream, t);
    else
      hipLaunchKernelGGL((ndt_batch_reduce_kernel<S>), dim3(static_cast<unsigned>(max_P), pairs), dim3(kThreads), 0, ctx->stream, t);
  }
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

// the round's launches of one kind of evaluation -> launches made
int enqueue_kind(dliom_ctx* ctx, int what, const char* table, int count, int max_n, int max_P, bool reduce, int64_t* launches) {
  if (count == 0 || (!reduce && max_n == 0)) return DLIOM_OK;  // empty sources evaluate to zeros: the leaves are never read
  if (launches != nullptr) {
    const int run = nn_batch_pairs_per_launch(std::max(max_n, 1));
    *launches += (count + run - 1) / run;
  }
  if (what == DLIOM_NDT_EVAL_ALL) return launch_kind<true, true>(ctx, table, count, max_n, max_P, reduce);
  if (what == DLIOM_NDT_EVAL_GRADIENT) return launch_kind<true, false>(ctx, table, count, max_n, max_P, reduce);
  return launch_kind<false, true>(ctx, table, count, max_n, max_P, reduce);
}

// One chunk: pairs [first, first + count) of the call, all in flight from its first round.
int run_chunk(Batch* b, const dliom_ndt_pair* pairs, int count, dliom_ndt_result* results, dliom_cloud** aligned) {
  dliom_ctx* ctx = b->ctx;
  const dliom_ndt_options* options = b->options;
  const NdtConstants constants = ndt_constants(*options);
  std::vector<Pair> chunk(static_cast<size_t>(count));
  size_t bytes = 0;
  for (int i = 0; i < count; ++i) bytes += pair_scratch_bytes(pairs[i].source->n);
  DLIOM_TRY(ctx->ndt_batch.reserve(bytes));
  char* const base = ctx->ndt_batch.as<char>();
  char* const table = base;
  char* const counters = base + kEntryBytes * static_cast<size_t>(count);
  char* at = counters + kCounterBytes * static_cast<size_t>(count);
  for (int i = 0; i < count; ++i) {
    Pair& p = chunk[i];
    p.in = &pairs[i];
    p.n = static_cast<int>(pairs[i].source->n);
    p.res.fitness_score = std::numeric_limits<double>::quiet_NaN();
    p.machine.start(*options, pairs[i].guess, &p.request);
    const Carve c = carve_of(p.n);
    NdtBatchEval& e = p.eval;
    std::memset(&e, 0, sizeof(e));
    e.table = ndt_table_of(pairs[i].target, constants);
    e.sx = pairs[i].source->d_x;
    e.sy = pairs[i].source->d_y;
    e.sz = pairs[i].source->d_z;
    e.leaves = reinterpret_cast<double*>(at + c.leaves);
    e.pairs = reinterpret_cast<int*>(at + c.pairs);
    e.partials = reinterpret_cast<double*>(at + c.partials);
    e.counts = reinterpret_cast<int*>(at + c.counts);
    e.n = p.n;
    e.P = c.P;
    e.P2 = c.P2;
    // the final round: ICP's arrays, as icp_batch.hip carves them
    NdtBatchFinal& f = p.last;
    std::memset(&f, 0, sizeof(f));
    f.searched = pairs[i].fitness_index != nullptr ? 1 : 0;
    if (f.searched != 0) nn_batch_item(pairs[i].fitness_index, DLIOM_NN_AUTO, &f.icp.nn);
    f.icp.P = c.P;
    f.icp.P2 = c.P2;
    char* const w = at + c.icp;
    const size_t per = align256(4 * static_cast<size_t>(std::max(p.n, 1)));
    int* const block = reinterpret_cast<int*>(counters + kCounterBytes * static_cast<size_t>(i));
    f.icp.max_sq = reinterpret_cast<unsigned*>(block) + 16;
    f.icp.nn.ox = reinterpret_cast<float*>(w);
    f.icp.nn.oy = reinterpret_cast<float*>(w + per);
    f.icp.nn.oz = reinterpret_cast<float*>(w + 2 * per);
    NnSearch& s = f.icp.nn.search;
    s.px = f.icp.nn.ox;
    s.py = f.icp.nn.oy;
    s.pz = f.icp.nn.oz;
    s.n = p.n;
    s.j = reinterpret_cast<int*>(w + 3 * per);
    s.d2 = reinterpret_cast<float*>(w + 4 * per);
    s.list = reinterpret_cast<int*>(w + 5 * per);
    s.key = reinterpret_cast<unsigned long long*>(w + 6 * per);
    s.counters = block;
    f.icp.partials = reinterpret_cast<double*>(w + 8 * per);
    f.icp.counts = reinterpret_cast<int*>(w + 8 * per + align256(static_cast<size_t>(c.P2) * kIcpSums * sizeof(double)));
    f.icp.nn.max_d2 = std::numeric_limits<double>::infinity();
    f.icp.nn.transform = 1;
    f.icp.nn.sx = e.sx;
    f.icp.nn.sy = e.sy;
    f.icp.nn.sz = e.sz;
    f.icp.want_norm = aligned != nullptr && p.n > 0 ? 1 : 0;
    at += c.total;
  }
  const FillJob fill{counters, kCounterBytes * static_cast<size_t>(count), 0u};  // every pair's counters and norm word
  DLIOM_TRY(fill_multi(ctx, &fill, 1));

  char* const host_table = pinned_at<char>(ctx, kPinNdtBatchTable);
  char* const host_slots = pinned_at<char>(ctx, kPinNdtBatchReadback);
  std::vector<int> active(static_cast<size_t>(count));
  for (int i = 0; i < count; ++i) active[i] = i;
  const int kinds[3] = {DLIOM_NDT_EVAL_ALL, DLIOM_NDT_EVAL_GRADIENT, DLIOM_NDT_EVAL_HESSIAN};
  while (!active.empty()) {
    const auto host_from = std::chrono::steady_clock::now();
    // the round's table: evaluations by kind, then the final rounds, the searched ones first
    std::vector<int> order;
    order.reserve(active.size());
    int kind_count[3] = {0, 0, 0}, kind_n[3] = {0, 0, 0}, kind_P[3] = {1, 1, 1};
    for (int k = 0; k < 3; ++k)
      for (int i : active) {
        const Pair& p = chunk[i];
        if (p.aligned || p.request.what != kinds[k]) continue;
        order.push_back(i);
        ++kind_count[k];
        kind_n[k] = std::max(kind_n[k], p.n);
        kind_P[k] = std::max(kind_P[k], p.eval.P);
      }
    const int evals = static_cast<int>(order.size());
    int searched = 0, finals_n = 0, searched_n = 0, normed_n = 0, max_segments = 1, searched_P = 1;
    for (int pass = 1; pass >= 0; --pass)
      for (int i : active) {
        const Pair& p = chunk[i];
        if (!p.aligned || p.last.searched != pass) continue;
        order.push_back(i);
        finals_n = std::max(finals_n, p.n);
        if (p.last.icp.want_norm != 0) normed_n = std::max(normed_n, p.n);
        if (pass == 1) {
          ++searched;
          searched_n = std::max(searched_n, p.n);
          searched_P = std::max(searched_P, p.last.icp.P);
          max_segments = std::max(max_segments, p.last.icp.nn.segments);
        }
      }
    const int A = static_cast<int>(order.size()), finals = A - evals;
    for (int a = 0; a < A; ++a) {
      Pair& p = chunk[order[a]];
      char* const to = host_table + kEntryBytes * static_cast<size_t>(a);
      if (a < evals) {
        ndt_pose(p.request.p, &p.eval.pose);
        p.eval.what = p.request.what;
        std::memcpy(to, &p.eval, sizeof(p.eval));
      } else {
        p.last.icp.slot = a;
        std::memcpy(to, &p.last, sizeof(p.last));
      }
    }
    b->host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_from).count();

    DLIOM_TRY(b->events->mark());
    DLIOM_HIP_TRY(hipMemcpyAsync(table, host_table, kEntryBytes * static_cast<size_t>(A), hipMemcpyHostToDevice, ctx->stream));
    int kinds_launched = 0;
    const char* t = table;
    for (int k = 0; k < 3; ++k) {
      const int64_t before = b->stats->evaluation_launches[kinds[k]];
      DLIOM_TRY(enqueue_kind(ctx, kinds[k], t, kind_count[k], kind_n[k], kind_P[k], false, &b->stats->evaluation_launches[kinds[k]]));
      if (b->stats->evaluation_launches[kinds[k]] != before) ++kinds_launched;
      t += kEntryBytes * static_cast<size_t>(kind_count[k]);
    }
    DLIOM_TRY(b->events->mark());
    t = table;
    for (int k = 0; k < 3; ++k) {
      DLIOM_TRY(enqueue_kind(ctx, kinds[k], t, kind_count[k], kind_n[k], kind_P[k], true, nullptr));
      t += kEntryBytes * static_cast<size_t>(kind_count[k]);
    }
    if (evals > 0) {
      hipLaunchKernelGGL(ndt_batch_finish_kernel, dim3(static_cast<unsigned>(evals)), dim3(kThreads), 0, ctx->stream, table, host_slots);
      DLIOM_HIP_TRY(hipGetLastError());
    }
    DLIOM_TRY(b->events->mark());
    if (finals > 0) {
      const char* const ft = table + kEntryBytes * static_cast<size_t>(evals);
      DLIOM_TRY(nn_transform_batch_enqueue(ctx, ft, kEntryBytes, finals, finals_n));
      if (normed_n > 0) {
        const int run = nn_batch_pairs_per_launch(normed_n);
        for (int first = 0; first < finals; first += run)
          hipLaunchKernelGGL(ndt_batch_max_norm_kernel, dim3(blocks_of(normed_n, kThreads), static_cast<unsigned>(std::min(run, finals - first))),
                             dim3(kThreads), 0, ctx->stream, ft + kEntryBytes * static_cast<size_t>(first));
        DLIOM_HIP_TRY(hipGetLastError());
      }
      if (searched > 0) {
        DLIOM_TRY(nn_search_batch_enqueue(ctx, ft, kEntryBytes, searched, searched_n, max_segments));
        hipLaunchKernelGGL(ndt_batch_fitness_reduce_kernel, dim3(static_cast<unsigned>(searched_P), static_cast<unsigned>(searched)),
                           dim3(kThreads), 0, ctx->stream, ft);
      }
      hipLaunchKernelGGL(ndt_batch_final_finish_kernel, dim3(static_cast<unsigned>(finals)), dim3(kThreads), 0, ctx->stream, ft,
                         host_slots + kSlotBytes * static_cast<size_t>(evals));
      DLIOM_HIP_TRY(hipGetLastError());
    }
    DLIOM_TRY(b->events->mark());
    const unsigned seq = next_done_seq(ctx);
    const auto enqueued_at = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(ndt_batch_done_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->done_word, seq);
    DLIOM_HIP_TRY(hipGetLastError());
    DLIOM_TRY(wait_done(ctx, ctx->stream, ctx->done_word, seq, b->poll_us));
    const auto took = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - enqueued_at).count();
    b->poll_us = static_cast<int>(std::min<long long>(std::max<long long>(2 * took, 150), 100000));
    ++b->stats->steps;
    ++b->stats->read_backs;
    b->stats->pair_evaluations += evals;
    b->stats->pair_searches += finals;
    if (kinds_launched + (finals > 0 ? 1 : 0) > 1) ++b->stats->mixed_steps;

    // the host's part: every pair's decision, then the list of the next round
    const auto decide_from = std::chrono::steady_clock::now();
    std::vector<int> next;
    next.reserve(active.size());
    for (int a = 0; a < A; ++a) {
      const int i = order[a];
      Pair& p = chunk[i];
      ++p.res.read_backs;
      const char* const slot = host_slots + kSlotBytes * static_cast<size_t>(a);
      if (a < evals) {
        NdtReadback rb;
        std::memcpy(&rb, slot, sizeof(rb));
        ndt_unpack(rb, p.request.what, &p.sums);
        if (p.machine.advance(p.sums, &p.request)) {
          next.push_back(i);
          continue;
        }
        NdtPose P;
        p.machine.finish(p.n, &p.res, &P);
        p.aligned = true;
        if (p.in->fitness_index != nullptr || aligned != nullptr) {  // one more round
          for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) p.last.icp.nn.m.m[4 * r + c] = P.R[3 * r + c];
            p.last.icp.nn.m.m[4 * r + 3] = P.t[r];
          }
          next.push_back(i);
          continue;
        }
        results[i] = p.res;
        continue;
      }
      IcpReadback rb;
      std::memcpy(&rb, slot, sizeof(rb));
      if (p.last.searched != 0) {
        p.res.fitness_count = rb.n;
        if (rb.n > 0) p.res.fitness_score = rb.sums[15] / static_cast<double>(rb.n);
      }
      results[i] = p.res;
      if (aligned != nullptr) {  // copied out of the chunk's scratch on the stream; the chunk's end waits for it
        float *x, *y, *z;
        DLIOM_TRY(alloc_device_cloud(ctx, p.n, &aligned[i], &x, &y, &z));
        float max_sq;
        std::memcpy(&max_sq, &rb.max_sq, 4);
        DLIOM_TRY(finish_device_cloud_from(ctx, aligned[i], std::sqrt(max_sq), p.last.icp.nn.ox, p.last.icp.nn.oy, p.last.icp.nn.oz));
      }
    }
    // the next round keeps the input order
    std::sort(next.begin(), next.end());
    active.swap(next);
    b->host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - decide_from).count();
  }
  if (aligned != nullptr) {  // the scratch is free again
    ++ctx->host_syncs;
    ++b->stats->synchronizations;
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return DLIOM_OK;
}

bool limits_ok(const dliom_ndt_batch_limits* l) {
  return l->max_pairs_in_flight >= 1 && l->max_pairs_in_flight <= DLIOM_NDT_BATCH_MAX_PAIRS && l->reserved == 0 && l->max_scratch_bytes > 0;
}

}  // namespace
}  // namespace dliom

extern "C" {

int64_t dliom_ndt_batch_scratch_bytes(int64_t source_points) {
  if (source_points < 0) return 0;
  return static_cast<int64_t>(dliom::pair_scratch_bytes(std::min<int64_t>(source_points, DLIOM_NN_MAX_POINTS)));
}

int dliom_ndt_batch_default_limits(dliom_ndt_batch_limits* limits) {
  if (limits == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *limits = dliom_ndt_batch_limits{64, 0, 64 * dliom_ndt_batch_scratch_bytes(DLIOM_NDT_BATCH_DEFAULT_POINTS)};
  return DLIOM_OK;
}

int dliom_ndt_align_batch(dliom_ctx* ctx, const dliom_ndt_pair* pairs, int count, const dliom_ndt_options* options,
                          const dliom_ndt_batch_limits* limits, dliom_ndt_result* results, dliom_cloud** aligned,
                          dliom_ndt_batch_stats* stats) {
  using namespace dliom;
  if (aligned != nullptr)
    for (int i = 0; i < count; ++i) aligned[i] = nullptr;
  dliom_ndt_batch_limits lim;
  (void)dliom_ndt_batch_default_limits(&lim);
  if (limits != nullptr) lim = *limits;
  if (ctx == nullptr || count < 0 || !ndt_options_ok(options) || !limits_ok(&lim)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (count > 0 && (pairs == nullptr || results == nullptr || ctx->done_word == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < count; ++i) {
    const dliom_ndt_pair& p = pairs[i];
    if (p.target == nullptr || p.source == nullptr || p.target->ctx != ctx || p.source->ctx != ctx || p.source->n < 0 ||
        p.source->n > DLIOM_NN_MAX_POINTS || (p.fitness_index != nullptr && nn_ctx(p.fitness_index) != ctx) || !ndt_guess_ok(p.guess) ||
        options->resolution != p.target->resolution)
      return DLIOM_ERR_INVALID_ARGUMENT;
  }
  dliom_ndt_batch_stats st = {};
  st.pairs = count;
  if (count == 0) {
    if (stats != nullptr) *stats = st;
    return DLIOM_OK;
  }
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  Events events{ctx, ctx->profiling, {}};
  Batch batch{ctx, options, &st, &events};
  int status = DLIOM_OK;
  for (int first = 0; first < count && status == DLIOM_OK;) {
    // dliom.h, Schedule: consecutive pairs until the chunk is full or the next pair's scratch would not fit
    int end = first;
    int64_t bytes = 0;
    while (end < count && end - first < lim.max_pairs_in_flight) {
      const int64_t need = dliom_ndt_batch_scratch_bytes(pairs[end].source->n);
      if (end > first && bytes + need > lim.max_scratch_bytes) break;
      bytes += need;
      ++end;
    }
    ++st.chunks;
    st.max_in_flight = std::max<int64_t>(st.max_in_flight, end - first);
    status = run_chunk(&batch, pairs + first, end - first, results + first, aligned != nullptr ? aligned + first : nullptr);
    first = end;
  }
  if (status == DLIOM_OK && !events.e.empty()) {
    ++ctx->host_syncs;
    ++st.synchronizations;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) status = DLIOM_ERR_HIP;
    for (size_t e = 0; status == DLIOM_OK && e + 3 < events.e.size(); e += 4) {
      float ms[3] = {0.f, 0.f, 0.f};
      for (int s = 0; s < 3; ++s)
        if (hipEventElapsedTime(&ms[s], events.e[e + s], events.e[e + s + 1]) != hipSuccess) status = DLIOM_ERR_HIP;
      st.evaluate_ms += ms[0];
      st.reduce_ms += ms[1];
      st.fitness_ms += ms[2];
    }
    st.host_ms = batch.host_ms;
  }
  if (status != DLIOM_OK) {  // no cloud is left behind
    (void)hipStreamSynchronize(ctx->stream);
    if (aligned != nullptr)
      for (int i = 0; i < count; ++i) {
        if (aligned[i] != nullptr) dliom_cloud_destroy(aligned[i]);
        aligned[i] = nullptr;
      }
    return status;
  }
  if (stats != nullptr) *stats = st;
  return DLIOM_OK;
}

}  // extern "C"
