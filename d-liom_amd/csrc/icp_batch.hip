// Many scan pairs aligned by ICP in one call (dliom.h "scan alignment by ICP", dliom_icp_align_batch): the loop of
// gen_ground_truth_by_ndt_match.cc:151-261, which aligns the two scans of every inter-submap constraint of a trajectory.
// The pairs of a chunk advance in lock step.  A step on the ACTIVE LIST -- the chunk's pairs that are not finished -- is
// one launch chain on the context's stream, with the pair as a grid dimension of every kernel:
//   the upload           the pairs' descriptors (IcpBatchEntry) from the page-locked table into HBM: one copy a step
//   nn_transform_batch_kernel (nn_index.hip)  the pairs that solved in the step before (in a pair's first step: its guess)
//   icp_batch_max_norm_kernel  the norm bound of the pairs in their fitness step, when the clouds are wanted
//   nn_shell / nn_brute / nn_resolve_batch_kernel (nn_index.hip)  every pair's search, with its own view, bound and counters
//   icp_batch_reduce_kernel  tree_reduce_kernel's tree, a workgroup per 2048 consecutive source indices of a pair
//   icp_batch_finish_kernel  a workgroup a pair: tree_finish over that pair's partial sums, into that pair's read-back slot
//   icp_batch_done_kernel    one completion word behind everything; the host polls it once (wait_done)
// Every kernel runs the body that the single call's kernel runs (nn_index.hip, tree_reduce.h, icp_internal.h) and the host
// decides with the single call's functions (icp_iterate and what it calls), so a pair's result has the single call's bits.
// A workgroup outside its pair's extent leaves as a whole before any barrier.  No floating-point atomics; the integer
// atomics (list counter, 64-bit key, statistics) are each pair's own.
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "device_common.h"
#include "icp_internal.h"

namespace dliom {
namespace {

constexpr int kThreads = kTreeThreads;
constexpr size_t kEntryBytes = kPinIcpBatchEntryBytes;
// what dliom_icp_batch_scratch_bytes counts in front of a pair's arrays: its descriptor (rounded up) and its counters
constexpr size_t kEntryShare = 512, kCounterBytes = 256;

static_assert(sizeof(IcpBatchEntry) <= kEntryBytes && kEntryBytes % 8 == 0 && kEntryBytes <= kEntryShare, "a descriptor fits its place");

// the bodies are icp_internal.h's: ndt_batch.hip runs them in its pairs' final rounds
__global__ __launch_bounds__(kThreads) void icp_batch_max_norm_kernel(const char* __restrict__ table) {
  icp_batch_max_norm_body(icp_batch_entry(table, kEntryBytes, blockIdx.y), static_cast<int>(blockIdx.x));
}

__global__ __launch_bounds__(kThreads) void icp_batch_reduce_kernel(const char* __restrict__ table) {
  icp_batch_reduce_body(icp_batch_entry(table, kEntryBytes, blockIdx.y), static_cast<int>(blockIdx.x));
}

__global__ __launch_bounds__(kThreads) void icp_batch_finish_kernel(const char* __restrict__ table, IcpReadback* slots) {
  const IcpBatchEntry& d = icp_batch_entry(table, kEntryBytes, blockIdx.x);
  icp_batch_finish_body(d, slots + d.slot);
}

// Runs behind the finish kernel on the stream: every slot has been written and fenced when the word goes out.
__global__ void icp_batch_done_kernel(unsigned* done_word, unsigned done_seq) { batch_done_body(done_word, done_seq); }

size_t pair_scratch_bytes(int64_t n) { return kEntryShare + kCounterBytes + icp_work_bytes(n); }

// A pair of the chunk in flight: the single call's local variables
struct Pair {
  const dliom_icp_pair* in = nullptr;
  int n = 0;
  dliom_icp_result res = {};
  double previous_mse = std::numeric_limits<double>::infinity();
  int k = 1;             // the iteration its next search belongs to
  bool fitness = false;  // its next search is the fitness score's
  IcpBatchEntry entry;   // arrays, geometry; transform, bound, want_norm and slot are set a step
};

struct Events {  // four a step while profiling is on: upload and transform | search | reduce and read-back
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
  const dliom_icp_options* options;
  dliom_icp_batch_stats* stats;
  Events* events;
  int poll_us = 150;  // of the step's completion word: twice what the previous step took
};

// One chunk: pairs [first, first + count) of the call, all in flight from its first step.
int run_chunk(Batch* b, const dliom_icp_pair* pairs, int count, dliom_icp_result* results, dliom_cloud** aligned) {
  dliom_ctx* ctx = b->ctx;
  const dliom_icp_options* options = b->options;
  std::vector<Pair> chunk(static_cast<size_t>(count));
  size_t bytes = 0;
  for (int i = 0; i < count; ++i) bytes += pair_scratch_bytes(pairs[i].source->n);
  DLIOM_TRY(ctx->icp_batch.reserve(bytes));
  char* const base = ctx->icp_batch.as<char>();
  char* const table = base;
  char* const counters = base + kEntryShare * static_cast<size_t>(count);
  char* at = counters + kCounterBytes * static_cast<size_t>(count);
  for (int i = 0; i < count; ++i) {
    Pair& p = chunk[i];
    p.in = &pairs[i];
    p.n = static_cast<int>(pairs[i].source->n);
    std::memcpy(p.res.transform, pairs[i].guess, sizeof(p.res.transform));
    p.res.mse = std::numeric_limits<double>::infinity();
    p.res.fitness_score = std::numeric_limits<double>::quiet_NaN();
    IcpBatchEntry& e = p.entry;
    std::memset(&e, 0, sizeof(e));
    nn_batch_item(pairs[i].index, options->search, &e.nn);
    tree_geometry(p.n, &e.P, &e.P2);
    const size_t per = align256(4 * static_cast<size_t>(std::max(p.n, 1)));
    int* const block = reinterpret_cast<int*>(counters + kCounterBytes * static_cast<size_t>(i));
    e.max_sq = reinterpret_cast<unsigned*>(block) + 16;
    e.nn.ox = reinterpret_cast<float*>(at);
    e.nn.oy = reinterpret_cast<float*>(at + per);
    e.nn.oz = reinterpret_cast<float*>(at + 2 * per);
    NnSearch& s = e.nn.search;
    s.px = e.nn.ox;
    s.py = e.nn.oy;
    s.pz = e.nn.oz;
    s.n = p.n;
    s.j = reinterpret_cast<int*>(at + 3 * per);
    s.d2 = reinterpret_cast<float*>(at + 4 * per);
    s.list = reinterpret_cast<int*>(at + 5 * per);
    s.key = reinterpret_cast<unsigned long long*>(at + 6 * per);
    s.counters = block;
    e.partials = reinterpret_cast<double*>(at + 8 * per);
    e.counts = reinterpret_cast<int*>(at + 8 * per + align256(static_cast<size_t>(e.P2) * kIcpSums * sizeof(double)));
    at += icp_work_bytes(p.n);
    // the first step's transform: the guess, from the source cloud
    e.nn.transform = 1;
    e.nn.sx = pairs[i].source->d_x;
    e.nn.sy = pairs[i].source->d_y;
    e.nn.sz = pairs[i].source->d_z;
    std::memcpy(e.nn.m.m, pairs[i].guess, sizeof(e.nn.m.m));
  }
  const FillJob fill{counters, kCounterBytes * static_cast<size_t>(count), 0u};  // every pair's counters and norm word
  DLIOM_TRY(fill_multi(ctx, &fill, 1));

  const double D = options->max_correspondence_distance;
  char* const host_table = pinned_at<char>(ctx, kPinIcpBatchTable);
  IcpReadback* const host_slots = pinned_at<IcpReadback>(ctx, kPinIcpBatchReadback);
  std::vector<int> active(static_cast<size_t>(count));
  for (int i = 0; i < count; ++i) active[i] = i;
  double solve_ms = 0.0;
  while (!active.empty()) {
    const int A = static_cast<int>(active.size());
    int max_n = 0, max_moved = 0, max_normed = 0, max_segments = 1, max_P = 1;
    for (int a = 0; a < A; ++a) {
      Pair& p = chunk[active[a]];
      IcpBatchEntry& e = p.entry;
      e.nn.max_d2 = p.fitness ? std::numeric_limits<double>::infinity() : D * D;
      e.want_norm = p.fitness && aligned != nullptr && p.n > 0 ? 1 : 0;
      e.slot = a;
      std::memcpy(host_table + kEntryBytes * static_cast<size_t>(a), &e, sizeof(e));
      max_n = std::max(max_n, p.n);
      if (e.nn.transform != 0) max_moved = std::max(max_moved, p.n);
      if (e.want_norm != 0) max_normed = std::max(max_normed, p.n);
      max_segments = std::max(max_segments, e.nn.segments);
      max_P = std::max(max_P, e.P);
    }
    DLIOM_TRY(b->events->mark());
    DLIOM_HIP_TRY(hipMemcpyAsync(table, host_table, kEntryBytes * static_cast<size_t>(A), hipMemcpyHostToDevice, ctx->stream));
    DLIOM_TRY(nn_transform_batch_enqueue(ctx, table, kEntryBytes, A, max_moved));
    if (max_normed > 0) {
      const int run = nn_batch_pairs_per_launch(max_normed);
      for (int first = 0; first < A; first += run)
        hipLaunchKernelGGL(icp_batch_max_norm_kernel, dim3(blocks_of(max_normed, kThreads), static_cast<unsigned>(std::min(run, A - first))),
                           dim3(kThreads), 0, ctx->stream, table + kEntryBytes * static_cast<size_t>(first));
      DLIOM_HIP_TRY(hipGetLastError());
    }
    DLIOM_TRY(b->events->mark());
    DLIOM_TRY(nn_search_batch_enqueue(ctx, table, kEntryBytes, A, max_n, max_segments));
    DLIOM_TRY(b->events->mark());
    hipLaunchKernelGGL(icp_batch_reduce_kernel, dim3(static_cast<unsigned>(max_P), static_cast<unsigned>(A)), dim3(kThreads), 0, ctx->stream,
                       table);
    hipLaunchKernelGGL(icp_batch_finish_kernel, dim3(static_cast<unsigned>(A)), dim3(kThreads), 0, ctx->stream, table, host_slots);
    const unsigned seq = next_done_seq(ctx);
    const auto enqueued_at = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(icp_batch_done_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->done_word, seq);
    DLIOM_HIP_TRY(hipGetLastError());
    DLIOM_TRY(b->events->mark());
    DLIOM_TRY(wait_done(ctx, ctx->stream, ctx->done_word, seq, b->poll_us));
    const auto took = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - enqueued_at).count();
    b->poll_us = static_cast<int>(std::min<long long>(std::max<long long>(2 * took, 150), 100000));
    ++b->stats->steps;
    ++b->stats->read_backs;
    b->stats->pair_searches += A;

    // the host's part: every pair's solve and decision, then the list of the next step
    const auto solve_from = std::chrono::steady_clock::now();
    std::vector<int> next;
    next.reserve(active.size());
    for (int a = 0; a < A; ++a) {
      Pair& p = chunk[active[a]];
      const IcpReadback rb = host_slots[a];
      ++p.res.read_backs;
      p.entry.nn.transform = 0;
      if (!p.fitness) {
        double R[9], t[3];
        bool ends = false;
        if (!icp_iterate(options, rb.sums, rb.n, p.k, &p.previous_mse, &p.res, R, t, &ends)) {
          p.fitness = true;  // T and the points stay
        } else {
          p.entry.nn.transform = 1;  // in place, in the next step's chain
          p.entry.nn.sx = p.entry.nn.ox;
          p.entry.nn.sy = p.entry.nn.oy;
          p.entry.nn.sz = p.entry.nn.oz;
          p.entry.nn.m = rigid_of(R, t);
          p.fitness = ends;
          ++p.k;
        }
        next.push_back(active[a]);
        continue;
      }
      p.res.fitness_count = rb.n;
      if (rb.n > 0) p.res.fitness_score = rb.sums[15] / static_cast<double>(rb.n);
      p.res.settled_by_grid = rb.counters[kNnByGrid];
      p.res.settled_by_brute_force = rb.counters[kNnByBruteForce];
      results[active[a]] = p.res;
      if (aligned != nullptr) {  // copied out of the chunk's scratch on the stream; the chunk's end waits for it
        float *x, *y, *z;
        DLIOM_TRY(alloc_device_cloud(ctx, p.n, &aligned[active[a]], &x, &y, &z));
        float max_sq;
        std::memcpy(&max_sq, &rb.max_sq, 4);
        DLIOM_TRY(finish_device_cloud_from(ctx, aligned[active[a]], std::sqrt(max_sq), p.entry.nn.ox, p.entry.nn.oy, p.entry.nn.oz));
      }
    }
    active.swap(next);
    solve_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - solve_from).count();
  }
  if (b->events->timed) b->stats->solve_ms += solve_ms;
  if (aligned != nullptr) {  // the scratch is free again
    ++ctx->host_syncs;
    ++b->stats->synchronizations;
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  return DLIOM_OK;
}

bool limits_ok(const dliom_icp_batch_limits* l) {
  return l->max_pairs_in_flight >= 1 && l->max_pairs_in_flight <= DLIOM_ICP_BATCH_MAX_PAIRS && l->reserved == 0 && l->max_scratch_bytes > 0;
}

}  // namespace
}  // namespace dliom

extern "C" {

int dliom_icp_batch_default_limits(dliom_icp_batch_limits* limits) {
  if (limits == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *limits = dliom_icp_batch_limits{64, 0, int64_t{1} << 30};
  return DLIOM_OK;
}

int64_t dliom_icp_batch_scratch_bytes(int64_t source_points) {
  if (source_points < 0) return 0;
  return static_cast<int64_t>(dliom::pair_scratch_bytes(std::min<int64_t>(source_points, DLIOM_NN_MAX_POINTS)));
}

int dliom_icp_align_batch(dliom_ctx* ctx, const dliom_icp_pair* pairs, int count, const dliom_icp_options* options,
                          const dliom_icp_batch_limits* limits, dliom_icp_result* results, dliom_cloud** aligned,
                          dliom_icp_batch_stats* stats) {
  using namespace dliom;
  if (aligned != nullptr)
    for (int i = 0; i < count; ++i) aligned[i] = nullptr;
  dliom_icp_batch_limits lim;
  (void)dliom_icp_batch_default_limits(&lim);
  if (limits != nullptr) lim = *limits;
  if (ctx == nullptr || count < 0 || !icp_options_ok(options) || !limits_ok(&lim)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (count > 0 && (pairs == nullptr || results == nullptr || ctx->done_word == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < count; ++i) {
    const dliom_icp_pair& p = pairs[i];
    if (p.index == nullptr || p.source == nullptr || nn_ctx(p.index) != ctx || p.source->ctx != ctx || p.source->n < 0 ||
        p.source->n > DLIOM_NN_MAX_POINTS || !icp_guess_ok(p.guess))
      return DLIOM_ERR_INVALID_ARGUMENT;
  }
  dliom_icp_batch_stats st = {};
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
      const int64_t need = dliom_icp_batch_scratch_bytes(pairs[end].source->n);
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
      st.transform_ms += ms[0];
      st.search_ms += ms[1];
      st.reduce_ms += ms[2];
    }
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
