// Many nearest-neighbour indices built in one call (dliom.h "scan alignment by ICP", dliom_nn_index_create_batch): the
// fourth per-pair cost of the loop of gen_ground_truth_by_ndt_match.cc:151-261 -- every distinct ICP target's index
// (:199-200) and every NDT pair's fitness index (:219).  A chunk of clouds is one launch chain on the context's stream
// with the cloud's slot as a grid dimension of every per-point kernel:
//   the upload                  the clouds' descriptors (coordinates, length) from the page-locked table
//   one fill                    every cloud's box words: the low words to ~0, the high words and the count to 0
//   nn_box_batch_kernel         nn_box_body: every cloud's box and finite count -> ONE polled read-back, 8 words a cloud
//   the host                    nn_choose_grid for every cloud; one allocation an index (by_index | cell_start | sorted)
//   the upload                  the descriptors again, now with every index's grid and arrays
//   and, a cell run at a time (consecutive indices whose cells + 1 sum to at most max_cells_in_flight):
//     one memset                the run's populations and cursors
//     nn_count_batch_kernel     nn_count_body: every point's cell, the populations, the points in the cloud's order
//     hipcub exclusive sum      ONE scan over the concatenation of the run's cell arrays (cells + 1 entries an index)
//     nn_scatter_batch_kernel   nn_scatter_body from the scan, and every index's OWN cell_start: the scan's value minus
//                               its value at the index's first cell
//   ONE stream synchronisation.
// The bodies are the single build's (nn_index_internal.h), run on the cloud's own points with the cloud's own grid, so
// an index answers every query with the single build's bits.  The order of the points inside a cell is whatever the
// atomics give, as in the single build; no result depends on it.  A workgroup outside its cloud's extent leaves as a
// whole; integer atomics only; every loop's bound is known before it starts (there is no loop); nothing waits on another
// workgroup.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>

#include "nn_index_internal.h"

namespace dliom {
namespace {

constexpr int kThreads = kNnThreads;
static_assert(kPinNnIndexBatchIndices == DLIOM_NN_INDEX_BATCH_MAX_INDICES, "pinned_layout.h has a descriptor for each index in flight");

struct NnIbEntry {  // a cloud of the chunk; from `first_cell` on: what the second upload brings
  const float *x, *y, *z;
  int n;
  int first_cell;      // of its cell run's concatenation
  int* cell_of_point;  // n entries of the work space
  float4* by_index;    // the index's own arrays
  float4* sorted;
  int* cell_start;
  NnCells cells;
  int entries;         // cells + 1
  int pad[8];
};
static_assert(sizeof(NnIbEntry) == kPinNnIndexBatchEntryBytes, "a descriptor fills its place");

// ---- the kernels: blockIdx.y = the cloud's slot, blockIdx.x over the longest extent of the launch -----------------------------
// lo_words, hi_words: four words a slot (nn_box_body)
__global__ __launch_bounds__(kThreads) void nn_box_batch_kernel(const NnIbEntry* __restrict__ table, unsigned* __restrict__ lo_words,
                                                                unsigned* __restrict__ hi_words) {
  const NnIbEntry& d = table[blockIdx.y];
  const int block = static_cast<int>(blockIdx.x);
  if (block * kThreads >= d.n) return;
  nn_box_body(d.x, d.y, d.z, d.n, lo_words + 4 * blockIdx.y, hi_words + 4 * blockIdx.y, block);
}

// counts: the run's populations, index after index
__global__ __launch_bounds__(kThreads) void nn_count_batch_kernel(const NnIbEntry* __restrict__ table, int* __restrict__ counts) {
  const NnIbEntry& d = table[blockIdx.y];
  const int block = static_cast<int>(blockIdx.x);
  if (block * kThreads >= d.n) return;
  const NnCells g = d.cells;
  nn_count_body(d.x, d.y, d.z, d.n, g, d.cell_of_point, counts + d.first_cell, d.by_index, block);
}

// scan: the exclusive sum of the run's populations; a workgroup beyond the cloud's points AND the index's cells leaves
__global__ __launch_bounds__(kThreads) void nn_scatter_batch_kernel(const NnIbEntry* __restrict__ table, const int* __restrict__ scan,
                                                                    int* __restrict__ cursor) {
  const NnIbEntry& d = table[blockIdx.y];
  const int block = static_cast<int>(blockIdx.x);
  if (block * kThreads >= max(d.n, d.entries)) return;
  const int* const starts = scan + d.first_cell;
  const int before = starts[0];
  nn_scatter_body(d.x, d.y, d.z, d.n, d.cell_of_point, starts, before, cursor + d.first_cell, d.sorted, block);
  const int c = block * kThreads + static_cast<int>(threadIdx.x);
  if (c < d.entries) d.cell_start[c] = starts[c] - before;
}

struct Clock {  // the stages' times, on the host's clock: every stage ends in a wait or on the host
  bool on;
  std::chrono::steady_clock::time_point from;
  void start() {
    if (on) from = std::chrono::steady_clock::now();
  }
  void lap(double* ms) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    *ms += std::chrono::duration<double, std::milli>(now - from).count();
    from = now;
  }
};

struct IndexDeleter {
  void operator()(dliom_nn_index* p) const { dliom_nn_index_destroy(p); }
};
using IndexPtr = std::unique_ptr<dliom_nn_index, IndexDeleter>;

// A launch holds at most 2^30 lanes: slots [0, count) of a table go in runs of as many as `extent` lanes a slot allow.
template <class Launch>
void launch_slots(int count, int64_t extent, Launch launch) {
  const unsigned blocks = blocks_of(std::max<int64_t>(extent, 1), kThreads);
  const int per = std::max(1, (1 << 22) / static_cast<int>(blocks));
  for (int first = 0; first < count; first += per) launch(first, dim3(blocks, static_cast<unsigned>(std::min(per, count - first))));
}

// A chunk's chain: clouds [0, count) -> built[0, count)
int run_chain(dliom_ctx* ctx, const dliom_cloud* const* clouds, int count, double edge0, int search, int64_t max_cells,
              std::vector<IndexPtr>* built, dliom_nn_index_batch_stats* st) {
  Clock clock{ctx->profiling, {}};
  clock.start();
  hipStream_t stream = ctx->stream;
  const dim3 block(kThreads);
  NnIbEntry* const host_table = pinned_at<NnIbEntry>(ctx, kPinNnIndexBatchTable);
  const size_t table_bytes = align256(sizeof(NnIbEntry) * static_cast<size_t>(count));
  const size_t word_bytes = align256(16 * static_cast<size_t>(count));
  int longest = 0;
  for (int t = 0; t < count; ++t) {
    NnIbEntry e = {};
    e.x = clouds[t]->d_x;
    e.y = clouds[t]->d_y;
    e.z = clouds[t]->d_z;
    e.n = static_cast<int>(clouds[t]->n);
    host_table[t] = e;
    longest = std::max(longest, e.n);
  }
  // ---- the boxes: table | low words | high words
  DLIOM_TRY(ctx->nn_index_batch.reserve(table_bytes + 2 * word_bytes));
  st->scratch_bytes = std::max<int64_t>(st->scratch_bytes, static_cast<int64_t>(table_bytes + 2 * word_bytes));
  {
    char* const base = ctx->nn_index_batch.as<char>();
    NnIbEntry* const table = reinterpret_cast<NnIbEntry*>(base);
    unsigned* const lo_words = reinterpret_cast<unsigned*>(base + table_bytes);
    unsigned* const hi_words = reinterpret_cast<unsigned*>(base + table_bytes + word_bytes);
    DLIOM_HIP_TRY(hipMemcpyAsync(table, host_table, sizeof(NnIbEntry) * static_cast<size_t>(count), hipMemcpyHostToDevice, stream));
    const FillJob fills[2] = {{lo_words, 16 * static_cast<size_t>(count), 0xFFFFFFFFu}, {hi_words, 16 * static_cast<size_t>(count), 0u}};
    DLIOM_TRY(fill_multi(ctx, fills, 2));
    launch_slots(count, longest, [&](int first, dim3 grid) {
      hipLaunchKernelGGL(nn_box_batch_kernel, grid, block, 0, stream, table + first, lo_words + 4 * first, hi_words + 4 * first);
    });
    DLIOM_HIP_TRY(hipGetLastError());
    const GatherJob jobs[2] = {{lo_words, 4u * static_cast<unsigned>(count)}, {hi_words, 4u * static_cast<unsigned>(count)}};
    DLIOM_TRY(gather_and_wait(ctx, jobs, 2, pinned_at<unsigned>(ctx, kPinNnIndexBatchBoxes)));
    ++st->read_backs;
  }
  clock.lap(&st->box_ms);

  // ---- the grids and the indices.  Nothing of the work space is live here: the table is written again below
  const unsigned* const host_lo = pinned_at<unsigned>(ctx, kPinNnIndexBatchBoxes);
  const unsigned* const host_hi = host_lo + 4 * static_cast<size_t>(count);
  built->resize(static_cast<size_t>(count));
  std::vector<int> run_first;  // the cell runs: [run_first[r], run_first[r + 1])
  std::vector<int64_t> run_entries;
  size_t scan_bytes = 0, point_offset = 0;
  int64_t in_run = 0;
  for (int t = 0; t < count; ++t) {
    IndexPtr f(new dliom_nn_index());
    f->ctx = ctx;
    f->n_target = clouds[t]->n;
    f->search = search;
    if (host_hi[4 * t + 3] > static_cast<unsigned>(clouds[t]->n)) return DLIOM_ERR_INTERNAL;
    nn_set_grid(f.get(), host_lo + 4 * t, host_hi + 4 * t, edge0);
    const size_t cells = static_cast<size_t>(f->dims[0]) * f->dims[1] * f->dims[2];
    const size_t by = nn_by_index_bytes(f->n_target), cs = nn_cell_start_bytes(cells), so = nn_sorted_bytes(f->n_finite);
    DLIOM_TRY(f->slab.reserve(by + cs + so));
    char* const slab = f->slab.as<char>();
    f->by_index.p = slab;
    f->by_index.cap = by;
    f->cell_start.p = slab + by;
    f->cell_start.cap = cs;
    f->sorted.p = slab + by + cs;
    f->sorted.cap = so;
    const int64_t entries = static_cast<int64_t>(cells) + 1;
    if (t == 0 || in_run + entries > max_cells) {  // dliom.h, Schedule: a cell run closes when the next index's cells would not fit
      run_first.push_back(t);
      run_entries.push_back(0);
      in_run = 0;
    }
    NnIbEntry& e = host_table[t];
    e.first_cell = static_cast<int>(in_run);
    e.by_index = f->by_index.as<float4>();
    e.sorted = f->sorted.as<float4>();
    e.cell_start = f->cell_start.as<int>();
    e.cells = nn_cells_of(f.get());
    e.entries = static_cast<int>(entries);
    e.cell_of_point = reinterpret_cast<int*>(point_offset);  // an offset until the work space is reserved
    point_offset += 4 * static_cast<size_t>(e.n);
    in_run += entries;
    run_entries.back() = in_run;
    st->finite_points += f->n_finite;
    st->cells += static_cast<int64_t>(cells);
    (*built)[static_cast<size_t>(t)] = std::move(f);
  }
  run_first.push_back(count);
  const int64_t most_entries = *std::max_element(run_entries.begin(), run_entries.end());
  for (const int64_t entries : run_entries) {
    size_t tmp = 0;
    DLIOM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, static_cast<const int*>(nullptr), static_cast<int*>(nullptr),
                                                   static_cast<int>(entries), stream));
    scan_bytes = std::max(scan_bytes, tmp);
  }
  // table | cell of point | populations | cursors | the scan | the scan's storage
  const size_t per = align256(4 * static_cast<size_t>(most_entries));
  const size_t of_points = table_bytes, of_counts = of_points + align256(point_offset), of_scan = of_counts + 2 * per,
               of_tmp = of_scan + per, total = of_tmp + align256(scan_bytes);
  DLIOM_TRY(ctx->nn_index_batch.reserve(total));
  st->scratch_bytes = std::max<int64_t>(st->scratch_bytes, static_cast<int64_t>(total));
  char* const base = ctx->nn_index_batch.as<char>();
  for (int t = 0; t < count; ++t)
    host_table[t].cell_of_point = reinterpret_cast<int*>(base + of_points + reinterpret_cast<size_t>(host_table[t].cell_of_point));
  clock.lap(&st->alloc_ms);

  // ---- the counting sort, a cell run at a time
  NnIbEntry* const table = reinterpret_cast<NnIbEntry*>(base);
  DLIOM_HIP_TRY(hipMemcpyAsync(table, host_table, sizeof(NnIbEntry) * static_cast<size_t>(count), hipMemcpyHostToDevice, stream));
  int* const scan = reinterpret_cast<int*>(base + of_scan);
  for (size_t r = 0; r + 1 < run_first.size(); ++r) {
    const int first = run_first[r], indices = run_first[r + 1] - first;
    const size_t run_per = align256(4 * static_cast<size_t>(run_entries[r]));
    int* const counts = reinterpret_cast<int*>(base + of_counts);
    int* const cursor = reinterpret_cast<int*>(base + of_counts + run_per);
    int64_t run_longest = 0, run_widest = 0;
    for (int t = first; t < first + indices; ++t) {
      run_longest = std::max<int64_t>(run_longest, host_table[t].n);
      run_widest = std::max<int64_t>(run_widest, std::max(host_table[t].n, host_table[t].entries));
    }
    DLIOM_HIP_TRY(hipMemsetAsync(counts, 0, 2 * run_per, stream));
    launch_slots(indices, run_longest, [&](int at, dim3 grid) {
      hipLaunchKernelGGL(nn_count_batch_kernel, grid, block, 0, stream, table + first + at, counts);
    });
    DLIOM_HIP_TRY(hipGetLastError());
    size_t tmp = scan_bytes;
    DLIOM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(base + of_tmp, tmp, counts, scan, static_cast<int>(run_entries[r]), stream));
    launch_slots(indices, run_widest, [&](int at, dim3 grid) {
      hipLaunchKernelGGL(nn_scatter_batch_kernel, grid, block, 0, stream, table + first + at, scan, cursor);
    });
    DLIOM_HIP_TRY(hipGetLastError());
    ++st->cell_runs;
  }
  DLIOM_HIP_TRY(hipStreamSynchronize(stream));  // the table and the work space are free again; the clouds are the caller's
  ++ctx->host_syncs;
  ++st->synchronizations;
  clock.lap(&st->sort_ms);
  return DLIOM_OK;
}

bool limits_ok(const dliom_nn_index_batch_limits& l) {
  return l.max_indices_in_flight >= 1 && l.max_indices_in_flight <= DLIOM_NN_INDEX_BATCH_MAX_INDICES && l.reserved == 0 &&
         l.max_points_in_flight >= 1 && l.max_points_in_flight <= (int64_t{1} << 30) && l.max_cells_in_flight >= 1 &&
         l.max_cells_in_flight <= (int64_t{1} << 30);
}

}  // namespace
}  // namespace dliom

extern "C" {

int dliom_nn_index_batch_default_limits(dliom_nn_index_batch_limits* limits) {
  if (limits == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *limits = dliom_nn_index_batch_limits{64, 0, int64_t{64} * DLIOM_NDT_BATCH_DEFAULT_POINTS, int64_t{1} << 26};
  return DLIOM_OK;
}

int dliom_nn_index_create_batch(dliom_ctx* ctx, const dliom_cloud* const* clouds, int count, const dliom_nn_index_options* options,
                                const dliom_nn_index_batch_limits* limits, dliom_nn_index** out, dliom_nn_index_batch_stats* stats) {
  using namespace dliom;
  if (out != nullptr)
    for (int i = 0; i < count; ++i) out[i] = nullptr;
  dliom_nn_index_batch_limits lim;
  (void)dliom_nn_index_batch_default_limits(&lim);
  if (limits != nullptr) lim = *limits;
  double edge0 = 0.0;
  int search = DLIOM_NN_AUTO;
  if (ctx == nullptr || out == nullptr || count < 0 || !nn_index_options_ok(options, &edge0, &search) || !limits_ok(lim))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (count > 0 && (clouds == nullptr || ctx->done_word == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < count; ++i)
    if (clouds[i] == nullptr || clouds[i]->ctx != ctx || clouds[i]->n < 1 || clouds[i]->n > DLIOM_NN_MAX_POINTS)
      return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_nn_index_batch_stats st = {};
  st.indices = count;
  if (count == 0) {
    if (stats != nullptr) *stats = st;
    return DLIOM_OK;
  }
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  std::vector<IndexPtr> all;  // whatever leaves this call early destroys what was built
  all.reserve(static_cast<size_t>(count));
  int status = DLIOM_OK;
  for (int first = 0; first < count && status == DLIOM_OK;) {
    // dliom.h, Schedule: consecutive clouds until the chunk is full or the next cloud's points would not fit
    int end = first;
    int64_t points = 0;
    while (end < count && end - first < lim.max_indices_in_flight) {
      if (end > first && points + clouds[end]->n > lim.max_points_in_flight) break;
      points += clouds[end]->n;
      ++end;
    }
    ++st.chunks;
    st.points += points;
    st.max_in_flight = std::max<int64_t>(st.max_in_flight, end - first);
    std::vector<IndexPtr> built;
    status = run_chain(ctx, clouds + first, end - first, edge0, search, lim.max_cells_in_flight, &built, &st);
    if (status != DLIOM_OK) (void)hipStreamSynchronize(ctx->stream);  // nothing writes the chunk's indices any more
    for (IndexPtr& p : built) all.push_back(std::move(p));
    first = end;
  }
  if (status != DLIOM_OK) return status;  // `all` goes, every out[i] is NULL
  for (int i = 0; i < count; ++i) out[i] = all[static_cast<size_t>(i)].release();
  if (stats != nullptr) *stats = st;
  return DLIOM_OK;
}

}  // extern "C"
