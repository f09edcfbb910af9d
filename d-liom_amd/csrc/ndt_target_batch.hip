// Many NDT targets built in one call (dliom.h "scan alignment by NDT", dliom_ndt_target_create_batch): the target half of the
// loop of gen_ground_truth_by_ndt_match.cc:151-261 under `--method ndt`.  A chunk's clouds are treated as ONE concatenation
// of positions (cloud t's run starts at the sum of the runs in front of it), and the chunk is one launch chain on the
// context's stream with the target's slot as a grid dimension of every per-point kernel:
//   the upload                    the targets' descriptors (coordinates, length, first position) from the page-locked table
//   ndt_tb_key_kernel             a lane a point: ndt_key_kernel's key, and as the value slot << 24 | the index in its cloud
//   hipcub radix sort             stable, by key, bits 0-64 over the whole concatenation
//   hipcub radix sort             stable, by the value's slot bits (ceil(log2 targets) of them), carrying the position: the
//                                 order is then slot, key, ascending point index -- within every target dliom_ndt_target_create's
//   ndt_tb_gather_kernel          the keys and the point indices through the sorted positions
//     (a chunk of one target sorts once, straight into the final arrays, and skips the second sort and the gather)
//   ndt_tb_head_kernel            segment heads: a target's first position always starts a cell
//   hipcub inclusive sum          ONE scan numbers the chunk's cells
//   ndt_tb_counts_kernel          every target's cell count and kept count from the scan at its ends -> the first read-back
//   ndt_tb_bounds_kernel          each cell's first position (in its target's run), key and slot
//   ndt_tb_cell_sums_kernel       a workgroup a cell over the chunk's total: the fixed tree over its own target's coordinates
//   one copy, ndt_tb_done_kernel  first positions, keys and sums of all cells -> the second read-back
//   the per-cell step             on the host, in double, target by target (ndt.hip ndt_finish_cells)
//   the tables' copies            every target's own allocation; ONE stream synchronisation
// Every kernel runs the body that the single build's kernel runs (ndt_internal.h) on the target's own run, so a target has
// the single build's bits.  A workgroup outside its cloud's extent leaves as a whole; nothing waits on another workgroup;
// no floating-point atomics (the only shared word, a target's kept count, has at most one writer).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "icp_internal.h"
#include "ndt_internal.h"

namespace dliom {
namespace {

constexpr int kThreads = kNdtThreads;
constexpr int kIndexBits = 24;  // a point's index in its cloud, below its target's slot in a sorted value
static_assert(DLIOM_NN_MAX_POINTS <= (1 << kIndexBits) && DLIOM_NDT_TARGET_BATCH_MAX_TARGETS <= (1 << (32 - kIndexBits)),
              "slot and index share 32 bits");
static_assert(kPinNdtTargetBatchTargets == DLIOM_NDT_TARGET_BATCH_MAX_TARGETS, "pinned_layout.h has a descriptor for each target in flight");

struct NdtTbTarget {  // a target of the chunk: its cloud and its run of the concatenation
  const float *x, *y, *z;
  int n, start;
};
static_assert(sizeof(NdtTbTarget) == kPinNdtTargetBatchEntryBytes, "a descriptor fills its place");

// A chunk's work space.  [live] stays until the sums are read back; [early] is dead after the gather and [cells], which
// the first read-back sizes, lies over it.
struct NdtTbWork {
  // live
  NdtTbTarget* table;
  unsigned *kept, *before, *cells;  // a word a target: kept count | the scan in front of its run | its cell count
  unsigned long long* keys;         // sorted: slot, key
  int* sorted_index;
  unsigned *head, *inclusive;
  // early
  unsigned long long *keys_in, *keys_mid;
  unsigned *value_in, *value_mid, *value_out;
  int *iota, *position;
  void* tmp;
  // cells
  int* cell_first;  // a target's cells + 1 entries, target after target: cell c of slot t at c + t
  unsigned long long* cell_key;
  double* sums;
  int* cell_slot;
};

struct NdtTbCarve {
  size_t table, words, keys, sorted_index, head, inclusive, early;  // offsets of the live arrays; early: where the rest starts
  size_t keys_in, keys_mid, value_in, value_mid, value_out, iota, position, tmp, early_bytes;  // from `early`
  size_t total;
  size_t sort_bytes, sort2_bytes, scan_bytes;
};

// cells' arrays from `early`: the read-back's span [cell_first | cell_key | sums] first, cell_slot behind
struct NdtTbCells {
  size_t first, key, sums, span, slot, bytes;
};
NdtTbCells cells_carve(size_t cells, size_t targets) {
  NdtTbCells c;
  c.first = 0;
  c.key = align256(4 * (cells + targets));
  c.sums = c.key + align256(8 * cells);
  c.span = c.sums + 72 * cells;
  c.slot = align256(c.span);
  c.bytes = c.slot + align256(4 * cells);
  return c;
}

int slot_bits(int targets) {
  int bits = 0;
  while ((1 << bits) < targets) ++bits;
  return bits;
}

int carve(dliom_ctx* ctx, int64_t points, int targets, NdtTbCarve* c) {
  const int n = static_cast<int>(points);
  c->sort_bytes = c->sort2_bytes = c->scan_bytes = 0;
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, c->sort_bytes, static_cast<const unsigned long long*>(nullptr),
                                                   static_cast<unsigned long long*>(nullptr), static_cast<const unsigned*>(nullptr),
                                                   static_cast<unsigned*>(nullptr), n, 0, 64, ctx->stream));
  if (targets > 1)
    DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, c->sort2_bytes, static_cast<const unsigned*>(nullptr),
                                                     static_cast<unsigned*>(nullptr), static_cast<const int*>(nullptr),
                                                     static_cast<int*>(nullptr), n, kIndexBits, kIndexBits + slot_bits(targets), ctx->stream));
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, c->scan_bytes, static_cast<const unsigned*>(nullptr), static_cast<unsigned*>(nullptr), n,
                                                 ctx->stream));
  const size_t N = static_cast<size_t>(points), T = static_cast<size_t>(targets);
  const size_t per8 = align256(8 * N), per4 = align256(4 * N);
  c->table = 0;
  c->words = c->table + align256(sizeof(NdtTbTarget) * T);
  c->keys = c->words + 3 * align256(4 * T);
  c->sorted_index = c->keys + per8;
  c->head = c->sorted_index + per4;
  c->inclusive = c->head + per4;
  c->early = c->inclusive + per4;
  c->keys_in = 0;
  c->keys_mid = c->keys_in + per8;
  c->value_in = c->keys_mid + per8;
  c->value_mid = c->value_in + per4;
  c->value_out = c->value_mid + per4;
  c->iota = c->value_out + per4;
  c->position = c->iota + per4;
  c->tmp = c->position + per4;
  c->early_bytes = c->tmp + align256(std::max(std::max(c->sort_bytes, c->sort2_bytes), c->scan_bytes));
  // every kept point may be a cell of its own
  c->total = c->early + std::max(c->early_bytes, cells_carve(N, T).bytes);
  return DLIOM_OK;
}

// ---- the kernels: blockIdx.y = the target's slot, blockIdx.x over the chunk's longest cloud -----------------------------------
__global__ __launch_bounds__(kThreads) void ndt_tb_key_kernel(const NdtTbTarget* __restrict__ table, float inv,
                                                              unsigned long long* __restrict__ keys, unsigned* __restrict__ value,
                                                              int* __restrict__ iota, unsigned* __restrict__ kept) {
  const NdtTbTarget d = table[blockIdx.y];
  if (static_cast<int>(blockIdx.x) * kThreads >= d.n) return;
  const int i = static_cast<int>(blockIdx.x) * kThreads + threadIdx.x;
  if (i == 0) kept[blockIdx.y] = static_cast<unsigned>(d.n);
  if (i >= d.n) return;
  const int at = d.start + i;
  keys[at] = ndt_key_body(d.x, d.y, d.z, i, inv);
  value[at] = (static_cast<unsigned>(blockIdx.y) << kIndexBits) | static_cast<unsigned>(i);
  iota[at] = at;
}

// position: where the concatenation's sorted position came from in the first sort's output
__global__ __launch_bounds__(kThreads) void ndt_tb_gather_kernel(int total, const int* __restrict__ position,
                                                                 const unsigned long long* __restrict__ keys_mid,
                                                                 const unsigned* __restrict__ value_mid,
                                                                 unsigned long long* __restrict__ keys, int* __restrict__ sorted_index) {
  const long long at = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
  if (at >= total) return;
  const int from = position[at];
  keys[at] = keys_mid[from];
  sorted_index[at] = static_cast<int>(value_mid[from] & ((1u << kIndexBits) - 1u));
}

__global__ __launch_bounds__(kThreads) void ndt_tb_head_kernel(const NdtTbTarget* __restrict__ table,
                                                               const unsigned long long* __restrict__ keys, unsigned* __restrict__ head,
                                                               unsigned* __restrict__ kept) {
  const NdtTbTarget d = table[blockIdx.y];
  const int i = static_cast<int>(blockIdx.x) * kThreads + threadIdx.x;
  if (i < d.n) ndt_head_body(keys + d.start, i, head + d.start, kept + blockIdx.y);
}

// One workgroup, a lane a target: the scan at the target's ends.  out (page-locked): cell count, kept count a target.
__global__ __launch_bounds__(kThreads) void ndt_tb_counts_kernel(const NdtTbTarget* __restrict__ table, int targets,
                                                                 const unsigned* __restrict__ inclusive, const unsigned* __restrict__ kept,
                                                                 unsigned* __restrict__ before, unsigned* __restrict__ cells, unsigned* out,
                                                                 unsigned* done_word, unsigned done_seq) {
  const int t = static_cast<int>(threadIdx.x);
  if (t < targets) {
    const NdtTbTarget d = table[t];
    const unsigned lo = d.start > 0 ? inclusive[d.start - 1] : 0u;
    const unsigned hi = inclusive[d.start + d.n - 1];
    before[t] = lo;
    cells[t] = hi - lo;
    out[2 * t] = hi - lo;
    out[2 * t + 1] = kept[t];
  }
  __threadfence_system();
  __syncthreads();
  batch_done_body(done_word, done_seq);
}

__global__ __launch_bounds__(kThreads) void ndt_tb_bounds_kernel(const NdtTbTarget* __restrict__ table,
                                                                 const unsigned long long* __restrict__ keys, const unsigned* __restrict__ head,
                                                                 const unsigned* __restrict__ inclusive, const unsigned* __restrict__ kept,
                                                                 const unsigned* __restrict__ before, const unsigned* __restrict__ cells,
                                                                 int* __restrict__ cell_first, unsigned long long* __restrict__ cell_key,
                                                                 int* __restrict__ cell_slot) {
  const NdtTbTarget d = table[blockIdx.y];
  if (static_cast<int>(blockIdx.x) * kThreads >= d.n) return;
  const int i = static_cast<int>(blockIdx.x) * kThreads + threadIdx.x;
  const unsigned base = before[blockIdx.y];
  const int count = static_cast<int>(cells[blockIdx.y]);
  ndt_bounds_body(keys + d.start, head + d.start, inclusive + d.start, base, i, d.n, count, static_cast<int>(kept[blockIdx.y]),
                  cell_first + base + blockIdx.y, cell_key + base);
  if (i < d.n && head[d.start + i] != 0u) {
    const int c = static_cast<int>(inclusive[d.start + i] - base) - 1;
    if (c >= 0 && c < count) cell_slot[base + c] = static_cast<int>(blockIdx.y);
  }
}

// a workgroup a cell of the chunk; sums: 9 a cell
__global__ __launch_bounds__(kThreads) void ndt_tb_cell_sums_kernel(const NdtTbTarget* __restrict__ table,
                                                                    const int* __restrict__ sorted_index, const int* __restrict__ cell_first,
                                                                    const int* __restrict__ cell_slot, double* __restrict__ sums) {
  const size_t c = blockIdx.x;
  const int t = cell_slot[c];
  const NdtTbTarget d = table[t];
  const int first = cell_first[c + t];
  ndt_cell_sums_body(d.x, d.y, d.z, sorted_index + d.start, first, cell_first[c + t + 1] - first, sums + c * 9);
}

__global__ void ndt_tb_done_kernel(unsigned* done_word, unsigned done_seq) { batch_done_body(done_word, done_seq); }

struct Clock {  // the stages' times, on the host's clock: every stage ends in a wait
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

// What a chunk holds on the host while its chain runs: the targets until the chunk has succeeded, the second read-back
// and the valid cells that the tables' copies read
struct Chunk {
  std::vector<std::unique_ptr<dliom_ndt_target>> t;
  std::vector<char> host;
  std::vector<NdtValidCells> valid;
  ~Chunk() {
    for (auto& p : t)
      if (p) p->table.release();
  }
};

// A chunk's chain: clouds [0, count) -> built->t[0, count)
int run_chain(dliom_ctx* ctx, const dliom_cloud* const* clouds, int count, const dliom_ndt_options* options, Chunk* built,
              dliom_ndt_target_batch_stats* st) {
  Clock clock{ctx->profiling, {}};
  clock.start();
  NdtTbTarget* const host_table = pinned_at<NdtTbTarget>(ctx, kPinNdtTargetBatchTable);
  int64_t points = 0;
  int longest = 0;
  for (int t = 0; t < count; ++t) {
    const int n = static_cast<int>(clouds[t]->n);
    host_table[t] = NdtTbTarget{clouds[t]->d_x, clouds[t]->d_y, clouds[t]->d_z, n, static_cast<int>(points)};
    points += n;
    longest = std::max(longest, n);
  }
  const int N = static_cast<int>(points);  // the schedule closes a chunk at 2^30 points, and a cloud alone is at most 2^24
  NdtTbCarve c;
  DLIOM_TRY(carve(ctx, points, count, &c));
  DLIOM_TRY(ctx->ndt_target_batch.reserve(c.total));
  st->scratch_bytes = std::max<int64_t>(st->scratch_bytes, static_cast<int64_t>(c.total));
  char* const base = ctx->ndt_target_batch.as<char>();
  char* const early = base + c.early;
  NdtTbWork w;
  w.table = reinterpret_cast<NdtTbTarget*>(base + c.table);
  const size_t word_bytes = align256(4 * static_cast<size_t>(count));
  w.kept = reinterpret_cast<unsigned*>(base + c.words);
  w.before = reinterpret_cast<unsigned*>(base + c.words + word_bytes);
  w.cells = reinterpret_cast<unsigned*>(base + c.words + 2 * word_bytes);
  w.keys = reinterpret_cast<unsigned long long*>(base + c.keys);
  w.sorted_index = reinterpret_cast<int*>(base + c.sorted_index);
  w.head = reinterpret_cast<unsigned*>(base + c.head);
  w.inclusive = reinterpret_cast<unsigned*>(base + c.inclusive);
  w.keys_in = reinterpret_cast<unsigned long long*>(early + c.keys_in);
  w.keys_mid = reinterpret_cast<unsigned long long*>(early + c.keys_mid);
  w.value_in = reinterpret_cast<unsigned*>(early + c.value_in);
  w.value_mid = reinterpret_cast<unsigned*>(early + c.value_mid);
  w.value_out = reinterpret_cast<unsigned*>(early + c.value_out);
  w.iota = reinterpret_cast<int*>(early + c.iota);
  w.position = reinterpret_cast<int*>(early + c.position);
  w.tmp = early + c.tmp;

  hipStream_t stream = ctx->stream;
  DLIOM_HIP_TRY(hipMemcpyAsync(w.table, host_table, sizeof(NdtTbTarget) * static_cast<size_t>(count), hipMemcpyHostToDevice, stream));
  const float inv = 1.0f / static_cast<float>(options->resolution);
  const dim3 grid(blocks_of(longest, kThreads), static_cast<unsigned>(count)), block(kThreads);
  hipLaunchKernelGGL(ndt_tb_key_kernel, grid, block, 0, stream, w.table, inv, w.keys_in, w.value_in, w.iota, w.kept);
  DLIOM_HIP_TRY(hipGetLastError());
  if (count == 1) {  // the value is the point's index: the single build's sort
    DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(w.tmp, c.sort_bytes, w.keys_in, w.keys, w.value_in,
                                                     reinterpret_cast<unsigned*>(w.sorted_index), N, 0, 64, stream));
  } else {
    DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(w.tmp, c.sort_bytes, w.keys_in, w.keys_mid, w.value_in, w.value_mid, N, 0, 64, stream));
    DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(w.tmp, c.sort2_bytes, w.value_mid, w.value_out, w.iota, w.position, N, kIndexBits,
                                                     kIndexBits + slot_bits(count), stream));
    hipLaunchKernelGGL(ndt_tb_gather_kernel, dim3(blocks_of(N, kThreads)), block, 0, stream, N, w.position, w.keys_mid, w.value_mid, w.keys,
                       w.sorted_index);
    DLIOM_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(ndt_tb_head_kernel, grid, block, 0, stream, w.table, w.keys, w.head, w.kept);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipcub::DeviceScan::InclusiveSum(w.tmp, c.scan_bytes, w.head, w.inclusive, N, stream));
  unsigned* const words = pinned_at<unsigned>(ctx, kPinReadback);
  unsigned seq = next_done_seq(ctx);
  hipLaunchKernelGGL(ndt_tb_counts_kernel, dim3(1), block, 0, stream, w.table, count, w.inclusive, w.kept, w.before, w.cells, words,
                     ctx->done_word, seq);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_TRY(wait_done(ctx, stream, ctx->done_word, seq, 2000));
  ++st->read_backs;
  clock.lap(&st->sort_ms);

  built->t.resize(static_cast<size_t>(count));
  std::vector<size_t> first_cell(static_cast<size_t>(count) + 1, 0);
  for (int t = 0; t < count; ++t) {
    const int64_t cells = words[2 * t], kept = words[2 * t + 1];
    if (cells > clouds[t]->n || kept > clouds[t]->n || cells > kept) return DLIOM_ERR_INTERNAL;
    auto target = std::make_unique<dliom_ndt_target>();
    target->ctx = ctx;
    target->resolution = options->resolution;
    target->min_points = options->min_points_per_voxel;
    target->n_points = clouds[t]->n;
    target->n_kept = kept;
    built->t[t] = std::move(target);
    first_cell[t + 1] = first_cell[t] + static_cast<size_t>(cells);
    st->kept_points += kept;
  }
  const size_t total_cells = first_cell[count];
  std::vector<NdtValidCells>& valid = built->valid;
  std::vector<char>& host = built->host;
  valid.resize(static_cast<size_t>(count));
  if (total_cells > 0) {
    const NdtTbCells k = cells_carve(total_cells, static_cast<size_t>(count));
    w.cell_first = reinterpret_cast<int*>(early + k.first);
    w.cell_key = reinterpret_cast<unsigned long long*>(early + k.key);
    w.sums = reinterpret_cast<double*>(early + k.sums);
    w.cell_slot = reinterpret_cast<int*>(early + k.slot);
    hipLaunchKernelGGL(ndt_tb_bounds_kernel, grid, block, 0, stream, w.table, w.keys, w.head, w.inclusive, w.kept, w.before, w.cells,
                       w.cell_first, w.cell_key, w.cell_slot);
    DLIOM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ndt_tb_cell_sums_kernel, dim3(static_cast<unsigned>(total_cells)), block, 0, stream, w.table, w.sorted_index,
                       w.cell_first, w.cell_slot, w.sums);
    DLIOM_HIP_TRY(hipGetLastError());
    host.resize(k.span);
    DLIOM_HIP_TRY(hipMemcpyAsync(host.data(), early, k.span, hipMemcpyDeviceToHost, stream));
    seq = next_done_seq(ctx);
    hipLaunchKernelGGL(ndt_tb_done_kernel, dim3(1), dim3(64), 0, stream, ctx->done_word, seq);
    DLIOM_HIP_TRY(hipGetLastError());
    DLIOM_TRY(wait_done(ctx, stream, ctx->done_word, seq, 2000));
    ++st->read_backs;
    clock.lap(&st->sums_ms);
    const int* const h_first = reinterpret_cast<const int*>(host.data() + k.first);
    const auto* const h_key = reinterpret_cast<const unsigned long long*>(host.data() + k.key);
    const double* const h_sums = reinterpret_cast<const double*>(host.data() + k.sums);
    for (int t = 0; t < count; ++t) {
      const size_t at = first_cell[t];
      ndt_finish_cells(built->t[t].get(), static_cast<int>(first_cell[t + 1] - at), h_first + at + t, h_key + at, h_sums + at * 9, &valid[t]);
    }
    clock.lap(&st->host_ms);
  }
  const int64_t chunk_read_backs = total_cells > 0 ? 2 : 1;
  int status = DLIOM_OK;
  for (int t = 0; t < count && status == DLIOM_OK; ++t) {
    status = ndt_table_upload_enqueue(built->t[t].get(), valid[t]);
    built->t[t]->build_read_backs = chunk_read_backs;
    st->cells += static_cast<int64_t>(built->t[t]->cells.size());
    st->valid_cells += built->t[t]->n_valid;
  }
  if (hipStreamSynchronize(stream) != hipSuccess && status == DLIOM_OK) status = DLIOM_ERR_HIP;  // the host vectors and the work space are free again
  ++ctx->host_syncs;
  ++st->synchronizations;
  if (status != DLIOM_OK) return status;
  clock.lap(&st->upload_ms);
  return DLIOM_OK;
}

// One chunk: clouds [0, count) -> out[0, count), all NULL unless the chunk succeeds
int run_chunk(dliom_ctx* ctx, const dliom_cloud* const* clouds, int count, const dliom_ndt_options* options, dliom_ndt_target** out,
              dliom_ndt_target_batch_stats* st) {
  Chunk built;
  const int status = run_chain(ctx, clouds, count, options, &built, st);
  if (status != DLIOM_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // no copy reads or writes the chunk's host memory any more
    return status;
  }
  for (int t = 0; t < count; ++t) out[t] = built.t[t].release();
  return DLIOM_OK;
}

bool limits_ok(const dliom_ndt_target_batch_limits& l) {
  return l.max_targets_in_flight >= 1 && l.max_targets_in_flight <= DLIOM_NDT_TARGET_BATCH_MAX_TARGETS && l.reserved == 0 &&
         l.max_points_in_flight >= 1 && l.max_points_in_flight <= (int64_t{1} << 30);
}

}  // namespace
}  // namespace dliom

extern "C" {

int dliom_ndt_target_batch_default_limits(dliom_ndt_target_batch_limits* limits) {
  if (limits == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *limits = dliom_ndt_target_batch_limits{64, 0, int64_t{64} * DLIOM_NDT_BATCH_DEFAULT_POINTS};
  return DLIOM_OK;
}

int dliom_ndt_target_create_batch(dliom_ctx* ctx, const dliom_cloud* const* clouds, int count, const dliom_ndt_options* options,
                                  const dliom_ndt_target_batch_limits* limits, dliom_ndt_target** out,
                                  dliom_ndt_target_batch_stats* stats) {
  using namespace dliom;
  if (out != nullptr)
    for (int i = 0; i < count; ++i) out[i] = nullptr;
  dliom_ndt_target_batch_limits lim;
  (void)dliom_ndt_target_batch_default_limits(&lim);
  if (limits != nullptr) lim = *limits;
  if (ctx == nullptr || out == nullptr || count < 0 || !ndt_options_ok(options) || !limits_ok(lim)) return DLIOM_ERR_INVALID_ARGUMENT;
  if (count > 0 && (clouds == nullptr || ctx->done_word == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < count; ++i)
    if (clouds[i] == nullptr || clouds[i]->ctx != ctx || clouds[i]->n <= 0 || clouds[i]->n > DLIOM_NN_MAX_POINTS)
      return DLIOM_ERR_INVALID_ARGUMENT;
  dliom_ndt_target_batch_stats st = {};
  st.targets = count;
  if (count == 0) {
    if (stats != nullptr) *stats = st;
    return DLIOM_OK;
  }
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  int status = DLIOM_OK;
  for (int first = 0; first < count && status == DLIOM_OK;) {
    // dliom.h, Schedule: consecutive clouds until the chunk is full or the next cloud's points would not fit
    int end = first;
    int64_t points = 0;
    while (end < count && end - first < lim.max_targets_in_flight) {
      if (end > first && points + clouds[end]->n > lim.max_points_in_flight) break;
      points += clouds[end]->n;
      ++end;
    }
    ++st.chunks;
    st.points += points;
    st.max_in_flight = std::max<int64_t>(st.max_in_flight, end - first);
    status = run_chunk(ctx, clouds + first, end - first, options, out + first, &st);
    first = end;
  }
  if (status != DLIOM_OK) {  // no target is left behind
    (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < count; ++i) {
      if (out[i] != nullptr) dliom_ndt_target_destroy(out[i]);
      out[i] = nullptr;
    }
    return status;
  }
  if (stats != nullptr) *stats = st;
  return DLIOM_OK;
}

}  // extern "C"
