/* dliom.h -- C ABI of the MI355X-native scan-to-submap front end.
 *
 * Drop-in boundary for the hot path of peterWon/D-LIOM's
 * cartographer::mapping::LocalTrajectoryBuilder3D.
 * Every entry point names the reference interface it replaces; paths are
 * relative to /root/reference/src/cartographer/cartographer.  The library is
 * libdliom.so (d-liom_amd/csrc, hand-written HIP for gfx950); there is no CPU
 * fallback behind these calls -- without a GPU they return DLIOM_ERR_NO_DEVICE.
 *
 * Conventions
 *   pose      double[7] = [tx,ty,tz,qw,qx,qy,qz]  (order of CeresPose::Data,
 *             mapping/internal/optimization/ceres_pose.h:47-51)
 *   points    packed float xyz, 12-byte stride == std::vector<Eigen::Vector3f>::data()
 *             (sensor/point_cloud.h:32)
 *   block     one 8x8x8 uint16 leaf of the reference HybridGrid, z-major
 *             ((z<<3)+y<<3)+x  (mapping/3d/hybrid_grid.h:40-43,66-138), addressed
 *             by the voxel index of its (0,0,0) corner (a multiple of 8 per axis)
 *   status    every function returns int: 0 ok, negative = the reference's
 *             CHECK condition that would have aborted (glog CHECK -> error code,
 *             SURVEY.md 8b "error convention"); nothing aborts or throws.
 *   threads   a dliom_ctx owns one HIP stream and its scratch memory; calls on
 *             different contexts are concurrency-safe (CeresScanMatcher3D::Match
 *             is re-entered from pool threads, constraint_builder_3d.cc:320).
 *             Grids are not thread-safe, like HybridGrid.
 */
#ifndef DLIOM_H_
#define DLIOM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLIOM_OK 0
#define DLIOM_ERR_INVALID_ARGUMENT (-1) /* CHECK_NOTNULL (rtcsm_3d.cc:38, range_data_inserter_3d.cc:80) */
#define DLIOM_ERR_HIP (-2)              /* a HIP runtime call failed; see dliom_last_error() */
#define DLIOM_ERR_NO_DEVICE (-3)        /* no gfx950 device visible */
#define DLIOM_ERR_SCORE_NOT_POSITIVE (-4) /* CHECK_GT(score, 0.f) rtcsm_3d.cc:111 */
#define DLIOM_ERR_WEIGHTS (-5)          /* CHECK_EQ / CHECK_GT ceres_scan_matcher_3d.cc:89-92 */
#define DLIOM_ERR_GRID_EXTENT (-6)      /* CHECK_LE(new_bits, 8) hybrid_grid.h:389 */
#define DLIOM_ERR_RAY_TOO_LONG (-7)     /* CHECK_LT(num_samples, 1 << 15) range_data_inserter_3d.cc:38 */
#define DLIOM_ERR_EMPTY_CLOUD (-8)      /* division by size()==0 in ScoreCandidate / sqrt(N) scaling */
#define DLIOM_ERR_CAPACITY (-9)         /* caller-provided output buffer too small */
#define DLIOM_ERR_SOLVER (-10)          /* Ceres would report FAILURE (evaluation or invalid steps) */
#define DLIOM_ERR_INTERNAL (-13)        /* a device 'cannot happen' word is set (2D ray casting: CHECK_NE / CHECK_EQ ray_casting.cc:114-115,144-145) */
#define DLIOM_ERR_PEER_FAILED (-12)     /* sharded match: another rank failed before the exchange (it still took part) */

typedef struct dliom_ctx dliom_ctx;
typedef struct dliom_grid dliom_grid;
typedef struct dliom_cloud dliom_cloud;
typedef struct dliom_inserter dliom_inserter;

const char* dliom_status_string(int status);
/* Text of the last HIP failure on the calling thread ("" if none). */
const char* dliom_last_error(void);
/* Number of visible HIP devices (0 when there is none). */
int dliom_device_count(void);

/* ---- context ------------------------------------------------------------ */
int dliom_ctx_create(int device_id, dliom_ctx** out);
/* Same, but work is enqueued on a caller-owned hipStream_t (e.g. torch's). */
int dliom_ctx_create_on_stream(int device_id, void* hip_stream, dliom_ctx** out);
int dliom_ctx_destroy(dliom_ctx* ctx);
int dliom_ctx_synchronize(dliom_ctx* ctx);
int dliom_ctx_device(const dliom_ctx* ctx); /* the device id it was created on (-1 for NULL) */

/* ---- probability value tables (host; mapping/probability_values.cc:73-83) --
 * table[v] = ProbabilityToValue(ProbabilityFromOdds(odds * Odds(p(v)))) + 32768,
 * what RangeDataInserter3D's constructor builds for hit and miss
 * (mapping/3d/range_data_inserter_3d.cc:70-76 with odds = Odds(float(p))). */
int dliom_compute_lookup_table_to_apply_odds(float odds, uint16_t* table32768);
float dliom_odds(float probability);
/* ProbabilityToValue (mapping/probability_values.h:91-93). */
uint16_t dliom_probability_to_value(float probability);
/* kValueToProbability (probability_values.cc:67-68), 65536 floats. */
int dliom_value_to_probability_table(float* table65536);

/* ---- device HybridGrid (replaces mapping/3d/hybrid_grid.h:470-547) -------- */
int dliom_grid_create(dliom_ctx* ctx, float resolution, dliom_grid** out);
int dliom_grid_destroy(dliom_grid* grid);
int dliom_grid_resolution(const dliom_grid* grid, float* resolution);
/* DynamicGrid::bits_ the reference would have after the same writes
 * (hybrid_grid.h:255,387-405). */
int dliom_grid_bits(const dliom_grid* grid, int* bits);
/* The correlative matcher's dense mirror of this grid: *rebuilds = how often it was (re)built since the
 * grid was created -- once for a whole-grid mirror, once per excursion of the search out of the mirrored window for
 * grids beyond bits = 4 --, *bytes = its current size (0: none), *windowed = 1 if it covers a window of the grid. */
int dliom_grid_mirror_stats(const dliom_grid* grid, int64_t* rebuilds, int64_t* bytes, int* windowed);
/* HBM accounting (no reference counterpart: the reference's grids live in host memory).  What a context's grids hold --
 * leaf tables ((8 << bits)^3 words), leaf pools (1 KiB + 12 B a leaf slot), the correlative matcher's dense mirrors
 * (272 MB at bits = 3, 2.2 GB at bits = 4, up to 4.04 GB for a window beyond that) -- and the
 * context's scratch buffers; nothing here synchronises with the device.  dliom_grid_memory_stats: one grid's share
 * (grids = 1, scratch_bytes = 0) with its leaf capacity and the host's upper bound of the slots in use.
 * dliom_ctx_set_mirror_budget: a cap on the sum of the context's mirrors (0 = none, the default).  A mirror that would
 * exceed it is not built and RealTimeCorrelativeScanMatcher3D runs its leaf-table kernel on that grid -- the same
 * results, several times slower (dliom_rtcsm_stats.box_kernel_status = DLIOM_BOX_REFUSED_NO_MIRROR, mirrors_refused
 * counts); mirrors that exist stay. */
typedef struct dliom_memory_stats {
  int64_t grids;
  int64_t leaf_table_bytes, leaf_pool_bytes, mirror_bytes;
  int64_t mirror_budget_bytes, mirrors_refused;
  int64_t scratch_bytes;           /* context only */
  int64_t leaf_capacity;           /* grid only: slots of the pool */
  int64_t leaf_slots_upper_bound;  /* grid only: >= slots in use (exact after dliom_grid_num_blocks) */
  int mirror_windowed;             /* grid only */
  int64_t outlier_table_bytes;     /* context only: the voxel tables of its dliom_outlier_remover objects */
  int64_t probability_grid_bytes;  /* the dense cells, tables and words of dliom_probability_grid objects (2D) */
  int64_t points_xray_bytes;       /* context only: tables and scratch of its dliom_points_xray objects */
} dliom_memory_stats;
int dliom_ctx_memory_stats(const dliom_ctx* ctx, dliom_memory_stats* out);
int dliom_ctx_set_mirror_budget(dliom_ctx* ctx, int64_t bytes);
int dliom_grid_memory_stats(const dliom_grid* grid, dliom_memory_stats* out);
/* Overwrites whole leaves; grows like mutable_value()/Grow(). */
int dliom_grid_upload_blocks(dliom_grid* grid, const int32_t* block_origin_xyz,
                             const uint16_t* values512, int64_t num_blocks);
int dliom_grid_num_blocks(const dliom_grid* grid, int64_t* num_blocks);
/* Allocated leaves in unspecified order; *num_blocks <= capacity. */
int dliom_grid_download_blocks(const dliom_grid* grid, int32_t* block_origin_xyz,
                               uint16_t* values512, int64_t capacity, int64_t* num_blocks);
/* *mutable_value(cell) = value for n cells (HybridGrid::SetProbability with
 * value = ProbabilityToValue(p), hybrid_grid.h:489-491; also how HybridGrid(proto) loads cells,
 * hybrid_grid.h:475-486).  Grows / allocates like the reference. */
int dliom_grid_set_values(dliom_grid* grid, const int32_t* cell_xyz, const uint16_t* values, int64_t n);
/* mapping::proto::HybridGrid wire bytes (mapping/proto/3d/hybrid_grid.proto) of the grid -- what
 * HybridGrid::ToProto().SerializeAsString() yields (hybrid_grid.h:530-542: cells in iterator order) --
 * and back (the proto constructor, hybrid_grid.h:475-486: SetProbability(ValueToProbability(v)) per
 * entry).  buffer == NULL queries *size.  This is how finished submaps leave / enter the device for
 * pbstream files and Submap3D::ToProto / UpdateFromProto (submap_3d.cc:217-250). */
int dliom_grid_to_proto(const dliom_grid* grid, uint8_t* buffer, int64_t capacity, int64_t* size);
int dliom_grid_from_proto(dliom_ctx* ctx, const uint8_t* buffer, int64_t size, dliom_grid** out);
/* mapping::proto::Submap3D (mapping/proto/submap.proto) around two serialized HybridGrid messages -- the message
 * Submap3D::ToProto fills (submap_3d.cc:217-230: local_pose, num_range_data, finished, the grids when
 * include_probability_grid_data) and the Submap3D(proto) constructor / UpdateFromProto read (:207-215,232-250).
 * Host only; the grid bytes come from / go to dliom_grid_to_proto / dliom_grid_from_proto.
 *   to_proto    *_grid_proto == NULL: that grid is absent (include_probability_grid_data == false);
 *               wrap_in_submap != 0: the bytes of proto::Submap{submap_3d = ...} as Submap3D::ToProto(proto::Submap*) emits;
 *               scalar fields equal to zero are omitted as the C++ proto3 runtime does; buffer == NULL queries *size
 *   from_proto  the grids are returned as (offset, size) into `buffer`, size -1 = absent */
int dliom_submap3d_to_proto(const double local_pose7[7], int32_t num_range_data, int finished,
                            const uint8_t* high_resolution_grid_proto, int64_t high_size,
                            const uint8_t* low_resolution_grid_proto, int64_t low_size, int wrap_in_submap,
                            uint8_t* buffer, int64_t capacity, int64_t* size);
int dliom_submap3d_from_proto(const uint8_t* buffer, int64_t size, int wrapped_in_submap, double local_pose7[7],
                              int32_t* num_range_data, int* finished, int64_t* high_offset, int64_t* high_size,
                              int64_t* low_offset, int64_t* low_size);
/* ---- compressed point clouds and trajectory node data (sensor/compressed_point_cloud.cc:99-146, mapping/
 * trajectory_node.cc:27-69): the other half of a saved pose graph, from the clouds in HBM ----
 * kPrecision = 0.001f, 10 bits per coordinate inside a block, 23 bits per direction.
 *
 * Compress(cloud), N points in input order:
 *  1 Bound    every coordinate p of every point: |p| / 0.001f < 8388608.f, a float division and a float comparison, so
 *             NaN and +-inf fail it.  (The reference CHECKs max(|x|, |y|, |z|), :113, and aborts; here the cloud is
 *             refused, see below.)  The largest float that passes is 8388.607421875, which rounds to 8388607: no
 *             accepted float reaches 2^23, so Grow()'s CHECK_LE(new_bits, 8) cannot fire for an accepted cloud.
 *  2 Round    per axis q = lround(p / 0.001f) -- GetCellIndex's float division, then round half away from zero --
 *             block = q >> 10 (arithmetic: negative q round down, block in [-8192, 8191]) and off = q & 1023.
 *  3 Blocks   in HybridGridBase's iterator order (hybrid_grid.h:181-231, 306-374).  With X = block_x + 8192 in
 *             [0, 16384), Y and Z likewise, blocks are ordered lexicographically by the nine fields
 *               Z >> 6, Y >> 6, X >> 6,   (Z >> 3) & 7, (Y >> 3) & 7, (X >> 3) & 7,   Z & 7, Y & 7, X & 7
 *             -- 42 bits, z-major at each of the three levels; the order does not depend on how far the DynamicGrid
 *             had grown, since Grow() shifts every meta cell by the same amount.
 *  4 Inside   a block the points keep their input order; duplicates stay duplicates.
 *  5 Stream   point_data, int32: per block in that order `count, block_x, block_y, block_z`, then a word a point,
 *             (((off_z << 10) + off_y) << 10) + off_x.  B blocks: 4 B + N words, at most 5 N.  num_points = N.  The
 *             empty cloud has the empty stream.
 * Decompress(num_points, point_data): ReadNextPoint's walk (:79-97); every coordinate is
 * float(int32((block << 10) + off)) * 0.001f, one conversion and one float multiply ((block << 10) + off in 32-bit
 * two's complement).  The reference does not validate (TODO, :153); here DLIOM_ERR_INVALID_ARGUMENT, and nothing read
 * past the buffer, for: a block count <= 0, a stream that ends inside a header or inside a block, counts that do not
 * sum to num_points, trailing words, a point word outside [0, 2^30), num_points < 0.
 *
 * Wire format (proto3).  sensor::proto::CompressedPointCloud: field 1 num_points, an int32 varint, omitted when 0;
 * field 3 point_data, packed int32 varints (a negative word is sign-extended to 64 bits: 10 bytes), omitted when empty.
 * mapping::proto::TrajectoryNodeData: 1 timestamp (int64 varint); 2 gravity_alignment (Quaterniond: x, y, z, w as doubles
 * 1-4); 3, 4, 5 the filtered gravity-aligned, high and low resolution clouds, each always present as a sub-message, even
 * when empty; 6 rotational_scan_matcher_histogram (packed float, every element); 7 local_pose (Rigid3d: 1 translation,
 * 2 rotation, both always present).  Scalars that compare equal to zero are omitted (v == 0.0, so -0.0 is omitted as
 * well, where the C++ runtime compares bits).  Parsers accept the packed and the unpacked form of a repeated field,
 * skip unknown fields and take the last occurrence of a sub-message.
 *
 * The device path is the batched one (K clouds of one context: keys, a stable sort over the key bits in use, emission,
 * varint packing); a single cloud is a batch of one.  A NULL cloud is the empty cloud.  Sizes come back in one
 * read-back a call, not one a cloud.  Query-then-fill as dliom_grid_to_proto: an output pointer of NULL is a size
 * query (offsets filled); a capacity below offsets[k] fills the offsets and returns DLIOM_ERR_CAPACITY.  5 * the
 * batch's points words always suffice.  A cloud that fails the bound check refuses the whole call with
 * DLIOM_ERR_GRID_EXTENT (the blocks are a HybridGridBase): *first_refused is the lowest such cloud's index (-1
 * otherwise) and neither the data nor the offsets are written.  More than 2^26 points or 2^20 clouds a batch:
 * DLIOM_ERR_TOO_LARGE.
 *   clouds_compress           cloud c's stream is point_data[word_offsets[c], word_offsets[c + 1]); capacity in words
 *   cloud_compress            k = 1: *size words
 *   clouds_compress_to_proto  K complete CompressedPointCloud messages, cloud c's at bytes[byte_offsets[c], [c + 1])
 *   cloud_decompress          a device cloud like every other (bounds kept: max_norm and the per-axis maxima)
 *   compressed_point_cloud_to_proto / _from_proto   host only: frames / parses words the caller holds (*n words;
 *                             point_data NULL queries *n); from_proto does not validate the stream
 *   compressed_point_cloud_check     host only: DLIOM_OK for a stream Decompress accepts, else DLIOM_ERR_INVALID_ARGUMENT
 *   trajectory_nodes_data_to_proto   `count` nodes, all their clouds (NULL: empty) compressed as one batch -- what a
 *                             SerializeState loop calls; node i's message is bytes[byte_offsets[i], [i + 1]);
 *                             *first_refused is the node's index; histogram_size >= 0
 *   trajectory_node_data_to_proto    count = 1: *size bytes
 *   trajectory_node_data_from_proto  three new device clouds (the caller's to destroy; absent: empty), *histogram_size
 *                             floats (DLIOM_ERR_CAPACITY with the size if histogram_capacity is too small), poses as
 *                             (w, x, y, z) and (x, y, z, qw, qx, qy, qz), absent fields zero */
int dliom_clouds_compress(dliom_ctx* ctx, const dliom_cloud* const* clouds, int k, int32_t* point_data, int64_t capacity,
                          int64_t* word_offsets, int* first_refused);
int dliom_cloud_compress(dliom_ctx* ctx, const dliom_cloud* cloud, int32_t* point_data, int64_t capacity, int64_t* size);
int dliom_clouds_compress_to_proto(dliom_ctx* ctx, const dliom_cloud* const* clouds, int k, uint8_t* bytes, int64_t capacity,
                                   int64_t* byte_offsets, int* first_refused);
int dliom_cloud_decompress(dliom_ctx* ctx, int32_t num_points, const int32_t* point_data, int64_t n, dliom_cloud** out);
int dliom_cloud_from_compressed_proto(dliom_ctx* ctx, const uint8_t* bytes, int64_t size, dliom_cloud** out);
int dliom_compressed_point_cloud_to_proto(int32_t num_points, const int32_t* point_data, int64_t n, uint8_t* buffer,
                                          int64_t capacity, int64_t* size);
int dliom_compressed_point_cloud_from_proto(const uint8_t* bytes, int64_t size, int32_t* num_points, int32_t* point_data,
                                            int64_t capacity, int64_t* n);
int dliom_compressed_point_cloud_check(int32_t num_points, const int32_t* point_data, int64_t n);
typedef struct {
  int64_t timestamp;                /* common::ToUniversal(time) */
  double gravity_alignment_wxyz[4];
  const dliom_cloud* filtered_gravity_aligned; /* each may be NULL: the empty cloud */
  const dliom_cloud* high_resolution;
  const dliom_cloud* low_resolution;
  const float* histogram;           /* rotational_scan_matcher_histogram */
  int histogram_size;
  double local_pose7[7];            /* x, y, z, qw, qx, qy, qz */
} dliom_trajectory_node_data;
int dliom_trajectory_nodes_data_to_proto(dliom_ctx* ctx, const dliom_trajectory_node_data* nodes, int count, uint8_t* bytes,
                                         int64_t capacity, int64_t* byte_offsets, int* first_refused);
int dliom_trajectory_node_data_to_proto(dliom_ctx* ctx, int64_t timestamp, const double gravity_alignment_wxyz[4],
                                        const dliom_cloud* filtered_gravity_aligned, const dliom_cloud* high_resolution,
                                        const dliom_cloud* low_resolution, const float* histogram, int histogram_size,
                                        const double local_pose7[7], uint8_t* buffer, int64_t capacity, int64_t* size);
int dliom_trajectory_node_data_from_proto(dliom_ctx* ctx, const uint8_t* bytes, int64_t size, int64_t* timestamp,
                                          double gravity_alignment_wxyz[4], dliom_cloud** filtered_gravity_aligned,
                                          dliom_cloud** high_resolution, dliom_cloud** low_resolution, float* histogram,
                                          int histogram_capacity, int* histogram_size, double local_pose7[7]);
/* ---- node clouds kept in HBM: map cloud messages and NodeRangeData (cartographer_ros/map_builder_bridge.cc:170-201,
 * 591-607, node.cc:203-220, 318-354, pb_range_data_to_ros_cloud_main.cc:153-186, msg_conversion.cc:159-171) ----
 * A cache keeps every scan's range_data_in_local (returns, misses) where the scan matcher left it.  Points are stored
 * SoA in pooled slabs; a node never straddles a slab and growth never moves an earlier node.  The descriptor table
 * (slab pointers, counts, prefix sums) lives on the host and is mirrored to the device by the first batched call that
 * needs it.  add is one kernel on the context's stream and waits for nothing: with pose_to_local the float pose is
 * applied on the way in (sensor::TransformPointCloud: rotation * p + translation in Eigen's operation order, as
 * dliom_cloud_download_transformed), to returns and misses alike; info->origin_in_local is kept as given.  The clouds
 * must be the cache's context's.  create_sized: floats a slab (<= 0: the default, 2^24); a node that needs more gets a
 * slab of its own.
 *
 * PointCloud2 data.  A record is the moved return and the float 1.0: x, y, z, 1.0f, 16 bytes, little endian; misses are
 * not part of it.  Poses are float (tx, ty, tz, qw, qx, qy, qz); two poses are applied one after the other, each
 * rounded as the reference rounds between them.  Node first + i's data is bytes[byte_offsets[i], byte_offsets[i + 1]),
 * 16 * its returns: the sizes are known on the host, so a chunk (whole nodes, at least one, up to
 * max_points_per_chunk returns) is one launch and one download, whatever the number of its nodes.
 *
 * mapping::proto::NodeRangeData (proto3).  1 timestamp (int64 varint), 2 trajectory_id, 3 node_index (int32 varints: a
 * negative value is sign-extended to ten bytes), each omitted when 0; 4 local_pose (Rigid3d: 1 translation, 2 rotation,
 * always present); 5 range_data_in_local (sensor::proto::RangeData, always present): 1 origin, always present, then
 * every return as a field 2 and every miss as a field 3, each a transform::proto::Vector3f sub-message: x, y, z as
 * fixed32 fields 1 to 3, a coordinate written unless v == 0 (so -0.0 is dropped and NaN is written, the rule of the
 * doubles above).  A point's record -- tag, length, payload -- is 2 to DLIOM_NODE_RANGE_MAX_RECORD bytes and lies at
 * any byte offset.  A chunk: one launch leaves the bytes of every tile of 256 records, one scan, ONE polled read-back
 * of the nodes' payload sizes (the host needs them for the two enclosing length varints and makes the headers), one
 * launch that writes headers and records, one download.  Framing (pbstream, gzip, SerializationHeader) is the caller's.
 * from_proto is a host parse and one upload a cloud: any field order, unknown fields skipped, absent fields zero,
 * repeated sub-messages merged as protobuf merges them; truncated or malformed input: DLIOM_ERR_INVALID_ARGUMENT.
 *
 * Conventions of dliom_trajectory_nodes_data_to_proto: byte_offsets (count + 1) are always filled; bytes NULL is a size
 * query; a capacity below byte_offsets[count] returns DLIOM_ERR_CAPACITY and nothing is written past capacity.  stats
 * (may be NULL): chunks, kernel launches (a scan counts as one), polled read-backs, points and bytes of the call.
 * DLIOM_ERR_INVALID_ARGUMENT: NULLs, a range outside the cache, num_poses outside 0..2, a cloud of another context. */
typedef struct dliom_node_clouds dliom_node_clouds;
typedef struct {
  int64_t timestamp;        /* common::ToUniversal(time) */
  int32_t trajectory_id;
  int32_t node_index;       /* SerializeRangeData never sets it: 0 there */
  double local_pose7[7];    /* x y z qw qx qy qz */
  float origin_in_local[3];
} dliom_node_cloud_info;
typedef struct {
  int64_t slabs, bytes_used, bytes_reserved; /* the point slabs */
  int64_t table_bytes;                       /* the descriptor table's device mirror */
  int64_t scratch_bytes;                     /* the batched calls' work buffers */
} dliom_node_clouds_memory;
typedef struct {
  int num_poses;        /* 0: the kept points as they are; 1: pose * p; 2: second * (first * p), two separate float transforms */
  int per_node;         /* 0: the same num_poses poses for every node; 1: num_poses poses per node, node-major */
  const float* poses7;  /* tx ty tz qw qx qy qz each */
} dliom_node_clouds_transform;
typedef struct { int64_t max_points_per_chunk; } dliom_node_clouds_limits;   /* <= 0: the default, 2^22 */
typedef struct { int chunks, launches, readbacks; int64_t points, bytes; } dliom_node_clouds_stats;
#define DLIOM_NODE_RANGE_MAX_RECORD 17
/* a message's bytes in front of its records never exceed this: a capacity of DLIOM_NODE_RANGE_MAX_HEADER a node and
 * DLIOM_NODE_RANGE_MAX_RECORD a point (returns and misses) NEVER returns DLIOM_ERR_CAPACITY -- one call, no size query */
#define DLIOM_NODE_RANGE_MAX_HEADER 192
int dliom_node_clouds_create(dliom_ctx* ctx, dliom_node_clouds** out);
int dliom_node_clouds_create_sized(dliom_ctx* ctx, int64_t slab_floats, dliom_node_clouds** out);
int dliom_node_clouds_destroy(dliom_node_clouds* clouds);
int dliom_node_clouds_clear(dliom_node_clouds* clouds);  /* forgets the nodes, keeps the first slab */
int dliom_node_clouds_add(dliom_node_clouds* clouds, const dliom_node_cloud_info* info, const dliom_cloud* returns,
                          const dliom_cloud* misses /* NULL: none */, const float pose_to_local[7] /* NULL: none */,
                          int64_t* index /* may be NULL */);
int dliom_node_clouds_size(const dliom_node_clouds* clouds, int64_t* nodes, int64_t* returns, int64_t* misses);
int dliom_node_clouds_info(const dliom_node_clouds* clouds, int64_t index, dliom_node_cloud_info* info, int64_t* num_returns,
                           int64_t* num_misses);
int dliom_node_clouds_memory_stats(const dliom_node_clouds* clouds, dliom_node_clouds_memory* memory);
/* packed xyz of one node (either pointer may be NULL); waits for the stream */
int dliom_node_clouds_download(const dliom_node_clouds* clouds, int64_t index, float* returns_xyz, float* misses_xyz);
int dliom_node_clouds_pack_point_cloud2(dliom_node_clouds* clouds, int64_t first, int64_t count,
                                        const dliom_node_clouds_transform* transform /* NULL: num_poses 0 */,
                                        const dliom_node_clouds_limits* limits /* NULL: defaults */, uint8_t* bytes,
                                        int64_t capacity, int64_t* byte_offsets /* count + 1 */, dliom_node_clouds_stats* stats);
/* the same records of one device cloud: *num_bytes = 16 n always; bytes NULL: the size only */
int dliom_cloud_pack_point_cloud2(const dliom_cloud* cloud, const float pose[7] /* or NULL */, uint8_t* bytes, int64_t capacity,
                                  int64_t* num_bytes);
/* host: Rigid3f::inverse (rigid_transform.h:167-171) in float: the conjugate, then -(conjugate * translation) */
int dliom_rigid3f_inverse(const float pose[7], float inverse[7]);
int dliom_node_clouds_to_proto(dliom_node_clouds* clouds, int64_t first, int64_t count, const dliom_node_clouds_limits* limits,
                               uint8_t* bytes, int64_t capacity, int64_t* byte_offsets /* count + 1 */,
                               dliom_node_clouds_stats* stats);
/* host only: the parse alone -- DLIOM_OK for a message from_proto accepts; info and the counts may be NULL */
int dliom_node_range_data_check(const uint8_t* bytes, int64_t size, dliom_node_cloud_info* info, int64_t* num_returns,
                                int64_t* num_misses);
/* two new device clouds, the caller's to destroy */
int dliom_node_range_data_from_proto(dliom_ctx* ctx, const uint8_t* bytes, int64_t size, dliom_node_cloud_info* info,
                                     dliom_cloud** returns, dliom_cloud** misses);
/* ---- gzip on the device (common::FastGzipString's place: submap_3d.cc:172, proto_stream.cc:50-57) ----
 * The last byte transformation before the wire, where the bytes already are.  zlib's stream cannot be reproduced in
 * parallel and no consumer needs it -- both readers only inflate -- so the encoder is stated here, the device equals
 * the host model of this statement (dliom_gzip_host) bit for bit, and zlib pins it as a decoder: the compressed bytes
 * are PARITY UNPINNED AGAINST ZLIB.  Output depends on every rule below.
 *  Member   1f 8b 08 00 00 00 00 00 04 03, the deflate stream, CRC-32 of the input and n mod 2^32, little-endian.
 *  Chunks   the input is cut into chunks of DLIOM_GZIP_CHUNK bytes, the last may be shorter, empty input is one empty
 *           chunk.  Chunks are independent: no match reaches before its chunk's first byte.  Every chunk's encoding
 *           starts and ends on a byte boundary.  The last chunk carries BFINAL = 1 on its last block.
 *  Tokens   of a chunk b[0, len), greedy, no lazy step, no distance penalty.  At position i <= len - 3 the candidate is
 *           the greatest j < i in the chunk with b[j, j + 3) == b[i, i + 3), taken over all positions, not only token
 *           starts.  L is the common prefix of b[j, ..) and b[i, ..), capped at min(258, len - i); overlap is allowed.
 *           L >= 3: emit (length L, distance i - j) and continue at i + L; otherwise literal b[i] and continue at i + 1.
 *  Fixed    one BTYPE = 01 block (RFC 1951's fixed codes, length 258 as code 285), then an empty stored block: 3 header
 *           bits, zero padding to the byte, 00 00 ff ff.  An empty chunk has only the stored block.
 *  Stored   one stored block holding the chunk, len + 5 bytes; used exactly when that is strictly smaller than the fixed form.
 *  Bound    dliom_gzip_bound(n) = 18 + n + 5 * max(1, ceil(n / 4096)); a buffer of that size is never too small.
 * The device calls run one launch chain for up to 8190 segments (chunk kernel, scan, sizes, gather), ONE polled read-back
 * of the members' offsets and one download of exactly the compressed bytes; they wait for the stream.
 * Refusals: NULL arguments, negative sizes, descending offsets DLIOM_ERR_INVALID_ARGUMENT; a capacity below what is needed
 * DLIOM_ERR_CAPACITY with the sizes filled and nothing written past capacity; a segment above DLIOM_GZIP_MAX_SEGMENT bytes
 * DLIOM_ERR_TOO_LARGE. */
#define DLIOM_GZIP_CHUNK 4096
#define DLIOM_GZIP_MAX_SEGMENT INT64_C(2147483647)
typedef struct { int64_t chunks, chunks_stored, read_backs, bytes_downloaded; } dliom_gzip_stats;
int64_t dliom_gzip_bound(int64_t n);  /* host; -1 for n < 0 */
/* host, one thread: the statement itself.  *size is filled whenever the arguments are valid */
int dliom_gzip_host(const uint8_t* bytes, int64_t n, uint8_t* out, int64_t capacity, int64_t* size);
/* upload, compress, download; stats may be NULL */
int dliom_gzip(dliom_ctx* ctx, const uint8_t* bytes, int64_t n, uint8_t* out, int64_t capacity, int64_t* size, dliom_gzip_stats* stats);
/* k members back to back: segment s is bytes[offsets[s], offsets[s + 1]), its member out[out_offsets[s], out_offsets[s + 1]) */
int dliom_gzip_segments(dliom_ctx* ctx, const uint8_t* bytes, const int64_t* offsets /* k + 1 */, int64_t k, uint8_t* out,
                        int64_t capacity, int64_t* out_offsets /* k + 1 */, dliom_gzip_stats* stats);
/* dliom_node_clouds_to_proto with every message leaving HBM as ProtoStreamWriter::WriteProto writes it: the 8-byte
 * little-endian size of the gzip member, then the member; record i is bytes[byte_offsets[i], byte_offsets[i + 1]).  Chunked
 * by the same limits; a chunk's messages never reach the host uncompressed.  bytes must not be NULL (the sizes are known
 * only after the work); a capacity of 8 + dliom_gzip_bound(DLIOM_NODE_RANGE_MAX_HEADER + DLIOM_NODE_RANGE_MAX_RECORD *
 * points) a node never returns DLIOM_ERR_CAPACITY.  gzip_stats may be NULL. */
int dliom_node_clouds_to_pbstream(dliom_node_clouds* clouds, int64_t first, int64_t count, const dliom_node_clouds_limits* limits,
                                  uint8_t* bytes, int64_t capacity, int64_t* byte_offsets /* count + 1 */,
                                  dliom_node_clouds_stats* stats, dliom_gzip_stats* gzip_stats);
/* ---- X-ray projections of a grid (mapping/3d/submap_3d.cc), computed on the device from the leaf pool ----
 * Both reproduce the reference's float arithmetic byte for byte: the cells with ValueToProbability(v) >= 0.501 in
 * HybridGrid::Iterator order, each cell centre index * resolution transformed in float and rounded with
 * RoundToInt(c * resolution_inverse), a per-pixel float probability sum added in iterator order.
 * Sizes follow dliom_grid_to_proto: buffer == NULL is a size query (DLIOM_OK, sizes filled); a buffer smaller than
 * the image fills the sizes and returns DLIOM_ERR_CAPACITY; a NULL grid, pose or size pointer returns
 * DLIOM_ERR_INVALID_ARGUMENT.  A projection of more than DLIOM_XRAY_MAX_PIXELS pixels fills the sizes and returns
 * DLIOM_ERR_CAPACITY whatever the buffer.
 * Empty projection: when no cell reaches 0.501 the reference's bounding box stays at (INT_MAX, INT_MIN) and its size
 * computation overflows (undefined).  Here that is DLIOM_OK with width = height = 0 and nothing written.
 * Runs on the grid's context stream and synchronises it; one small read-back (the bounding box) sizes the image. */
#define DLIOM_XRAY_MAX_PIXELS (INT64_C(1) << 26)
/* Submap3D::ToResponseProto's AddToTextureProto (submap_3d.cc:53-177, 253-262) without the gzip step.
 *   cells        height * width (value, alpha) byte pairs, row (max_x - px), column (max_y - py): the texture's
 *                uncompressed `cells` (the caller applies common::FastGzipString); capacity in bytes
 *   width        max_y - min_y + 1, height max_x - min_x + 1 of the rounded xy indices
 *   resolution   the grid's (float) resolution
 *   slice_pose7  global_submap_pose.inverse() * Translation(max_x * res, max_y * res, global_submap_pose.z), the
 *                products in float widened to double (for an empty projection max_x = max_y = 0)
 * Poses are (tx, ty, tz, qw, qx, qy, qz); the cell transform is global_submap_pose.cast<float>(). */
int dliom_grid_xray_texture(const dliom_grid* grid, const double global_submap_pose7[7], uint8_t* cells, int64_t capacity,
                            int32_t* width, int32_t* height, double* resolution, double slice_pose7[7]);
/* ... with the gzip step (submap_3d.cc:172): `cells` leaves HBM as ONE gzip member of dliom.h "gzip on the device", ready
 * for the proto field, and never reaches the host uncompressed.  *cells_gz_size: the member's bytes; cells_gz NULL: the
 * sizes and *cells_gz_size = dliom_gzip_bound(2 * width * height), a capacity that never fails (the projection's first
 * phase runs, nothing is compressed).  An empty projection is the member of empty input.  gzip_stats may be NULL. */
int dliom_grid_xray_texture_gzip(const dliom_grid* grid, const double global_submap_pose7[7], uint8_t* cells_gz, int64_t capacity,
                                 int64_t* cells_gz_size, int32_t* width, int32_t* height, double* resolution, double slice_pose7[7],
                                 dliom_gzip_stats* gzip_stats);
/* D-LIOM's ProjectToCvMat (submap_3d.cc:381-443): the gravity-aligned, yaw-free top-down CV_8UC1 image for loop
 * detection.  The cells are rotated by Embed3D(Rigid2d::Rotation(-GetYaw(T))).cast<float>() *
 * Rigid3d::Rotation(T.rotation()).cast<float>() (no translation; transform.h:43-52, 110-115).
 *   image        height * width bytes, row-major: pixel (py - min_y) * width + (px - min_x); capacity in bytes
 *   width        max_x - min_x + 1, height max_y - min_y + 1; ox = min_x * resolution, oy = min_y * resolution (double)
 * Every pixel, empty ones included, is RoundToInt((probability_sum - 0.1f) * (255.f / 0.8f)) stored into a uchar,
 * i.e. reduced modulo 256, as the reference stores it before cv::threshold: an empty pixel is 224 and a column whose
 * sum exceeds ~0.9 wraps past 255.  This is the reference's behaviour, kept on purpose. */
int dliom_grid_project_to_image(const dliom_grid* grid, const double transform7[7], uint8_t* image, int64_t capacity,
                                int32_t* width, int32_t* height, double* ox, double* oy, double* resolution);
/* ProbabilityToLogOddsInteger (mapping/submaps.h:37-52, glibc logf) for probability in [0.1, 0.9], as the texture
 * kernel evaluates it: from a table of the 254 floats where the result steps up, built on the host when the
 * library loads (1 below 0.1, 255 above 0.9). */
uint8_t dliom_probability_to_log_odds_integer(float probability);
/* HybridGrid::value() for n cell indices (0 outside / unallocated). */
int dliom_grid_get_values(const dliom_grid* grid, const int32_t* cell_xyz, int64_t n,
                          uint16_t* values);
/* RangeDataInserter3D::Insert(range_data{origin, returns, {}}, grid)
 * (mapping/3d/range_data_inserter_3d.cc:78-92): hits with hit_table, then for
 * each ray the last num_free_space_voxels cells with miss_table, each cell at
 * most once per call, then FinishUpdate(). */
int dliom_grid_insert(dliom_grid* grid, const float origin[3], const float* returns_xyz,
                      int64_t num_returns, const uint16_t* hit_table32768,
                      const uint16_t* miss_table32768, int num_free_space_voxels);

/* ---- RangeDataInserter3D object (mapping/3d/range_data_inserter_3d.h:35-47) ---
 * The constructor builds the hit and miss odds tables once
 * (range_data_inserter_3d.cc:70-76) and keeps them in HBM. */
int dliom_inserter_create(dliom_ctx* ctx, double hit_probability, double miss_probability,
                          int num_free_space_voxels, dliom_inserter** out);
int dliom_inserter_destroy(dliom_inserter* inserter);
/* Host copies of hit_table_ / miss_table_ (32768 entries each; either may be NULL). */
int dliom_inserter_tables(const dliom_inserter* inserter, uint16_t* hit_table32768,
                          uint16_t* miss_table32768);
/* RangeDataInserter3D::Insert(RangeData{origin, returns, {}}, grid). */
int dliom_inserter_insert(const dliom_inserter* inserter, dliom_grid* grid, const float origin[3],
                          const float* returns_xyz, int64_t num_returns);
/* Submap3D::InsertRangeData's data path on the device (mapping/3d/submap_3d.cc:264-279):
 * sensor::TransformRangeData through num_poses (0..2) float poses applied in sequence
 * (poses7[k] = [tx,ty,tz,qw,qx,qy,qz]; e.g. tracking->local then local->submap), then
 * FilterRangeDataByMaxRange(max_range) when max_range > 0 (submap_3d.cc:42-51), then Insert.
 * `origin` is given in the cloud's own frame and is transformed the same way. */
int dliom_inserter_insert_cloud(const dliom_inserter* inserter, dliom_grid* grid,
                                const float* poses7, int num_poses, const float origin[3],
                                const dliom_cloud* cloud, float max_range);

/* The same for up to 4 grids in one set of launches -- the four insertions of
 * ActiveSubmaps3D::InsertRangeData (both grids of both active submaps, submap_3d.cc:303-309).
 * Target k uses poses7[14*k .. 14*k + 7*num_poses[k]) and max_range[k].
 * The insertion calls (this one, _insert_cloud, dliom_front_end_insert*) return as soon as the device has told the
 * host whether the grids can hold the scan (status, growth); the update passes themselves are still on the context's
 * stream then.  Every later call ON THE SAME CONTEXT is ordered behind them; the cloud may be destroyed right away
 * (dliom_cloud_destroy waits for the device).  Code that reads a grid through ANOTHER context (a loop-closure thread
 * building a matcher on an active submap) calls dliom_ctx_synchronize on the inserting context first -- finished
 * submaps handed out by dliom_front_end_take_finished_submap need nothing, they have been synchronised. */
int dliom_inserter_insert_cloud_multi(const dliom_inserter* inserter, int num_targets,
                                      dliom_grid* const* grids, const float* poses7, const int* num_poses,
                                      const float origin[3], const dliom_cloud* cloud,
                                      const float* max_range);

/* ---- device-resident point cloud (sensor::PointCloud staged in HBM) ------- */
int dliom_cloud_create(dliom_ctx* ctx, const float* points_xyz, int64_t n, dliom_cloud** out);
int dliom_cloud_destroy(dliom_cloud* cloud);
int dliom_cloud_size(const dliom_cloud* cloud, int64_t* n);
/* The bounds the cloud carries, as its producer left them (no device work, no synchronisation): max_norm = max_i |p_i|
 * (float, x*x + (y*y + z*z), a NaN norm never counts, 0 for an empty cloud) and abs_max = max_i |x_i|, |y_i|, |z_i| per
 * axis, or a negative value where the producer does not know it (max_norm bounds that axis then).  The matchers'
 * search windows and the inserters' growth are sized from these. */
int dliom_cloud_bounds(const dliom_cloud* cloud, float* max_norm, float abs_max[3]);

/* ---- RealTimeCorrelativeScanMatcher3D -------------------------------------
 * proto::RealTimeCorrelativeScanMatcherOptions
 * (mapping/proto/scan_matching/real_time_correlative_scan_matcher_options.proto) */
typedef struct dliom_rtcsm_options {
  double linear_search_window;
  double angular_search_window;
  double translation_delta_cost_weight;
  double rotation_delta_cost_weight;
} dliom_rtcsm_options;

/* float RealTimeCorrelativeScanMatcher3D::Match(initial_pose_estimate,
 * point_cloud, hybrid_grid, pose_estimate)
 * (mapping/internal/3d/scan_matching/real_time_correlative_scan_matcher_3d.h:47-50,
 *  .cc:34-53).  *score receives the returned best score. */
int dliom_rtcsm3d_match(dliom_ctx* ctx, const dliom_rtcsm_options* options,
                        const double initial_pose_estimate[7], const float* points_xyz,
                        int64_t n, const dliom_grid* grid, double pose_estimate[7],
                        float* score);
/* Same with the cloud already in HBM. */
int dliom_rtcsm3d_match_cloud(dliom_ctx* ctx, const dliom_rtcsm_options* options,
                              const double initial_pose_estimate[7], const dliom_cloud* cloud,
                              const dliom_grid* grid, double pose_estimate[7], float* score);

/* The same match with the search window sharded across GPUs (BASELINE config 4): every rank
 * holds the cloud and the grid, owns the rotations [shard*R/num_shards, (shard+1)*R/num_shards)
 * (all translations of each), and the ranks exchange two words:
 *   begin  -> local best score LOWER BOUND (float bits, non-negative: orders like an integer)
 *             ... all-reduce MAX over ranks ...
 *   finish <- that global bound; -> local winner packed as (score_bits << 32) | (0xFFFFFFFF - index)
 *             ... all-reduce MAX over ranks (the lower index wins ties, like the reference's
 *             first strictly greater score in generation order, rtcsm_3d.cc:46-51) ...
 *   decode <- the global word; -> pose_estimate and score, identical on every rank.
 * With num_shards == 1 the three calls equal dliom_rtcsm3d_match_cloud. */
int dliom_rtcsm3d_shard_begin(dliom_ctx* ctx, const dliom_rtcsm_options* options,
                              const double initial_pose_estimate[7], const dliom_cloud* cloud,
                              const dliom_grid* grid, int shard, int num_shards,
                              uint32_t* local_best_lower_bound_bits);
int dliom_rtcsm3d_shard_finish(dliom_ctx* ctx, uint32_t global_best_lower_bound_bits,
                               uint64_t* local_best_packed);
int dliom_rtcsm3d_shard_decode(dliom_ctx* ctx, uint64_t global_best_packed, double pose_estimate[7],
                               float* score);

/* Search-window geometry of the last/next match (rtcsm_3d.cc:58-70). */
typedef struct dliom_rtcsm_window {
  int linear_window_size;
  int angular_window_size;
  float angular_step_size;
  float max_scan_range;
  int64_t num_translations; /* (2L+1)^3 */
  int64_t num_rotations;    /* (2A+1)^3 */
  int64_t num_candidates;
} dliom_rtcsm_window;
int dliom_rtcsm3d_window(const dliom_rtcsm_options* options, float resolution,
                         const float* points_xyz, int64_t n, dliom_rtcsm_window* window);

/* Statistics of the last dliom_rtcsm3d_match* on this context. */
typedef struct dliom_rtcsm_stats {
  dliom_rtcsm_window window;
  int64_t num_points;
  int64_t num_rescored;   /* candidates re-scored with the sequential float sum */
  int64_t best_index;     /* generation order: ((z,y,x) * R + (rz,ry,rx)) */
  int64_t score_kernel;   /* score-volume kernel that ran: 3 LDS-box, 2 dense mirror, 1 rotation per lane over the leaf
                             table, 0 point per lane over the leaf table */
  int64_t box_kernel_status; /* why: DLIOM_BOX_* below (a refusal is not an error -- the other kernels give the same
                                bits 1.9 to 4.4 times slower -- but it should not go unnoticed) */
  int64_t box_kernel_variant; /* score_kernel == 3: which instantiation ran -- 0: 27 translations per pass at four waves per
                                 SIMD (one-pass windows), 1: the same at three waves per SIMD with larger boxes, 2: 49
                                 translations per pass (windows of many passes); -1 otherwise */
} dliom_rtcsm_stats;
enum {
  DLIOM_BOX_RAN = 0,               /* the LDS-box kernel scored the volume */
  DLIOM_BOX_NOT_REQUESTED = 1,     /* DLIOM_TUNE_SCORE_KERNEL chose another kernel */
  DLIOM_BOX_REFUSED_SMALL = 2,     /* fewer than 8 translations or 2^24 candidate-point pairs: launch-bound anyway */
  DLIOM_BOX_REFUSED_NO_MIRROR = 3, /* the grid has no dense mirror (bits >= 5, or no memory for it) */
  DLIOM_BOX_REFUSED_RANGE = 4,     /* the scan's range beyond the fast index's (max ||p|| / resolution > ~860 cells); the
                                      POSITION in the grid is not limited (any cell DynamicGrid addresses) */
  DLIOM_BOX_REFUSED_WINDOW = 5,    /* angular window x range: a typical point's lookups do not fit a box */
  DLIOM_BOX_REFUSED_LDS = 6,       /* the box + lists exceed the LDS budget */
  DLIOM_BOX_REFUSED_FLAGGED = 7    /* the box kernel flagged an inconsistency ("cannot happen"): this match was redone
                                      on the dense kernel (dliom_rtcsm3d_box_error holds the sticky flag) */
};
int dliom_rtcsm3d_last_stats(const dliom_ctx* ctx, dliom_rtcsm_stats* stats);
/* BASELINE config 4 in one call: this rank scores rotations [shard R / num_shards, (shard + 1) R / num_shards), finds its
 * own winner exactly, and ONE max all-reduce of one uint64 (score_bits << 32 | ~candidate_index) yields the reference's
 * winner on every rank (rtcsm_3d.cc:46-51: first strictly greater score in generation order).
 *   _sharded       the collective is the caller's: `exchange` replaces *value by the maximum over all ranks (0 = ok)
 *   _sharded_rccl  `nccl_comm` is an ncclComm_t (RCCL, resolved with dlopen at first use; rank and size come from the
 *                  communicator): ncclAllReduce(ncclMax, ncclUint64, count 1) on the context's stream
 * A rank whose local part fails still takes part in the exchange (it contributes the reserved word
 * 0x7FFFFFFFFFFFFFFF, above every real word under signed or unsigned MAX) and returns its own status afterwards;
 * every other rank returns DLIOM_ERR_PEER_FAILED.  No rank is ever left waiting in the collective. */
typedef int (*dliom_allreduce_max_u64)(uint64_t* value, void* user);
int dliom_rtcsm3d_match_sharded(dliom_ctx* ctx, const dliom_rtcsm_options* options, const double initial_pose_estimate[7],
                                const dliom_cloud* cloud, const dliom_grid* grid, int shard, int num_shards,
                                dliom_allreduce_max_u64 exchange, void* user, double pose_estimate[7], float* score);
int dliom_rtcsm3d_match_sharded_rccl(dliom_ctx* ctx, const dliom_rtcsm_options* options,
                                     const double initial_pose_estimate[7], const dliom_cloud* cloud, const dliom_grid* grid,
                                     void* nccl_comm, double pose_estimate[7], float* score);
/* Diagnostic: sticky consistency flags of the LDS-box score kernel on this context (0 = every exactly
 * resolved lookup fell inside its staged box, as the construction guarantees).  Synchronises. */
int dliom_rtcsm3d_box_error(dliom_ctx* ctx, uint32_t* flags);

/* ---- CeresScanMatcher3D ------------------------------------------------------
 * proto::CeresScanMatcherOptions3D + common.proto.CeresSolverOptions
 * (mapping/proto/scan_matching/ceres_scan_matcher_options_3d.proto,
 *  common/proto/ceres_solver_options.proto). */
#define DLIOM_MAX_CLOUDS 8
typedef struct dliom_csm_options {
  int num_occupied_space_weights;
  double occupied_space_weight[DLIOM_MAX_CLOUDS];
  double translation_weight;
  double rotation_weight;
  int only_optimize_yaw;
  int use_nonmonotonic_steps;
  int max_num_iterations;
  int num_threads; /* accepted, unused: the device evaluates all points at once */
} dliom_csm_options;

/* The fields of ceres::Solver::Summary the path reads
 * (local_trajectory_builder_3d.cc:543) plus evaluation counts. */
typedef struct dliom_csm_summary {
  double initial_cost;
  double final_cost;
  int num_successful_steps;
  int num_unsuccessful_steps;
  int num_iterations;
  int num_residual_evaluations;
  int num_jacobian_evaluations;
  int termination_type; /* 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE */
} dliom_csm_summary;

/* void CeresScanMatcher3D::Match(target_translation, initial_pose_estimate,
 * point_clouds_and_hybrid_grids, pose_estimate, summary)
 * (mapping/internal/3d/scan_matching/ceres_scan_matcher_3d.h:51-56, .cc:71-123). */
int dliom_csm3d_match(dliom_ctx* ctx, const dliom_csm_options* options,
                      const double target_translation[3], const double initial_pose_estimate[7],
                      int num_clouds, const float* const* points_xyz, const int64_t* n,
                      const dliom_grid* const* grids, double pose_estimate[7],
                      dliom_csm_summary* summary);
int dliom_csm3d_match_cloud(dliom_ctx* ctx, const dliom_csm_options* options,
                            const double target_translation[3],
                            const double initial_pose_estimate[7], int num_clouds,
                            const dliom_cloud* const* clouds, const dliom_grid* const* grids,
                            double pose_estimate[7], dliom_csm_summary* summary);
/* One CeresScanMatcher3D::Match of a batch (dliom_csm3d_match_batch): cloud j is clouds[j] when that is not NULL, else
 * the host points points_xyz[j] (n[j] of them). */
typedef struct dliom_batch_stats dliom_batch_stats;  /* below, with the batched loop-closure search */
typedef struct dliom_csm_problem {
  double target_translation[3];
  double initial_pose_estimate[7];
  int num_clouds;
  const float* points_xyz[DLIOM_MAX_CLOUDS];
  int64_t n[DLIOM_MAX_CLOUDS];
  const dliom_cloud* clouds[DLIOM_MAX_CLOUDS];
  const dliom_grid* grids[DLIOM_MAX_CLOUDS];
} dliom_csm_problem;
/* The refinement stage of a batch of loop-closure constraints (constraint_builder_3d.cc:311-320: one option set for
 * the batch).  poses[7 * i], summaries[i] (may be NULL) and statuses[i] = what dliom_csm3d_match of problems[i] gives,
 * bit for bit.  Problems up to DLIOM_TUNE_CSM_ONE_LAUNCH_MAX points run in ONE launch of csm_lm_batch_kernel (one
 * workgroup each, one completion word for all); larger ones take the single call's path.  NULL pointers (a grid, host
 * points with n > 0) or count < 0 fail the whole call with DLIOM_ERR_INVALID_ARGUMENT before anything runs. */
int dliom_csm3d_match_batch(dliom_ctx* ctx, const dliom_csm_options* options, int count, const dliom_csm_problem* problems,
                            double* poses, dliom_csm_summary* summaries, int* statuses, dliom_batch_stats* stats);

/* ---- scan-to-submap front end --------------------------------------------------------------
 * LocalTrajectoryBuilder3D::AddAccumulatedRangeData + InsertIntoSubmap
 * (mapping/internal/3d/local_trajectory_builder_3d.cc:493-622) around ActiveSubmaps3D
 * (mapping/3d/submap_3d.cc:281-326), WITHOUT the GTSAM window: the caller runs WindowOptimize
 * between dliom_front_end_match() and dliom_front_end_insert(), exactly where the reference does
 * (:555-557), and passes the optimised pose to insert. */
typedef struct dliom_front_end dliom_front_end;

typedef struct dliom_adaptive_voxel_filter_options { /* sensor/proto/adaptive_voxel_filter_options.proto */
  float max_length;
  float min_num_points;
  float max_range;
} dliom_adaptive_voxel_filter_options;

typedef struct dliom_front_end_options { /* proto/3d/local_trajectory_builder_options_3d.proto (subset) */
  dliom_adaptive_voxel_filter_options high_resolution_adaptive_voxel_filter;
  dliom_adaptive_voxel_filter_options low_resolution_adaptive_voxel_filter;
  int use_online_correlative_scan_matching;
  dliom_rtcsm_options real_time_correlative_scan_matcher;
  dliom_csm_options ceres_scan_matcher;
  /* proto/motion_filter_options.proto */
  double motion_filter_max_time_seconds;
  double motion_filter_max_distance_meters;
  double motion_filter_max_angle_radians;
  /* proto/3d/submaps_options_3d.proto */
  double high_resolution;
  double high_resolution_max_range;
  double low_resolution;
  int num_range_data;
  double hit_probability;
  double miss_probability;
  int num_free_space_voxels;
} dliom_front_end_options;

typedef struct dliom_match_result {
  int dropped;                        /* 1: the reference returns nullptr (:497-500,510-513,531-534) */
  double pose_estimate[7];            /* local frame: submap.local_pose * observation (:552-553) */
  double pose_observation_in_submap[7];
  double initial_ceres_pose[7];       /* after the optional RTCSM (:504-521) */
  float rtcsm_score;                  /* 0 when the online matcher is off */
  dliom_csm_summary summary;
  double residual_distance;           /* :544-547 */
  double residual_angle;              /* :548-551 */
  int64_t num_high_resolution_points; /* after the adaptive voxel filters (:506-509,526-530) */
  int64_t num_low_resolution_points;
  int matching_submap_index;
} dliom_match_result;

typedef struct dliom_insertion_result {
  int inserted;                 /* 0: MotionFilter::IsSimilar said "similar" (:593-595) */
  int num_insertion_submaps;    /* submaps the range data went into (1 or 2) */
  int insertion_submap_index[2];/* trajectory-wide submap indices */
  int submap_added;             /* a new submap was started after this insertion */
  int submap_finished;          /* the oldest active submap was finished and dropped */
} dliom_insertion_result;

int dliom_front_end_create(dliom_ctx* ctx, const dliom_front_end_options* options, dliom_front_end** out);
int dliom_front_end_destroy(dliom_front_end* fe);
/* filtered_range_data_in_tracking = {origin, returns} (misses are not used by the 3D path).
 * pose_prediction: tracking frame -> local frame. */
int dliom_front_end_match(dliom_front_end* fe, const double pose_prediction[7], const float origin[3],
                          const float* returns_xyz, int64_t num_returns, dliom_match_result* result);
/* The same with the range data already resident on the device (e.g. the output of
 * dliom_cloud_voxel_filter); `returns` must stay alive until the following dliom_front_end_insert. */
int dliom_front_end_match_cloud(dliom_front_end* fe, const double pose_prediction[7], const float origin[3],
                                const dliom_cloud* returns, dliom_match_result* result);
/* InsertIntoSubmap with the range data of the preceding match.  time_ticks: cartographer
 * common::Time ticks (100 ns).  gravity_alignment: quaternion (w,x,y,z) used for new submaps. */
int dliom_front_end_insert(dliom_front_end* fe, int64_t time_ticks, const double pose_estimate[7],
                           const double gravity_alignment[4], dliom_insertion_result* result);
/* ActiveSubmaps3D::submaps() / matching_index(). */
int dliom_front_end_num_active_submaps(const dliom_front_end* fe, int* n);
int dliom_front_end_matching_index(const dliom_front_end* fe, int* index);
/* ActiveSubmaps3D::InsertRangeData(range_data, gravity_alignment) (mapping/3d/submap_3d.h:111-112, .cc:296-314) on the
 * front end's active submaps: range data already in the LOCAL frame, no MotionFilter. */
int dliom_front_end_insert_range_data(dliom_front_end* fe, const float origin_in_local[3],
                                      const dliom_cloud* returns_in_local, const double gravity_alignment[4],
                                      dliom_insertion_result* result);
/* Finished submaps (Submap3D::Finish(), submap_3d.cc:316-326) leave the active pair but stay alive for the back end:
 * the reference hands them on as shared_ptr and drops them when the pose graph is done.  Here the front end holds
 * them (leaf pools shrunk to the leaves in use, dense mirror released) until the caller TAKES them, oldest first;
 * a taken submap's grids belong to the caller (dliom_grid_destroy).  Not taking them keeps every finished submap
 * resident. */
int dliom_front_end_num_finished_submaps(const dliom_front_end* fe, int* n);
int dliom_front_end_take_finished_submap(dliom_front_end* fe, double local_pose[7], int* num_range_data,
                                         dliom_grid** high_resolution_grid, dliom_grid** low_resolution_grid);
/* The adaptively filtered clouds of the last successful match, in the tracking frame -- TrajectoryNode::Data's
 * high_resolution_point_cloud / low_resolution_point_cloud (local_trajectory_builder_3d.cc:506-533,613-619).  Borrowed:
 * valid until the next match on this front end; NULL when the last match dropped its scan. */
int dliom_front_end_matched_clouds(const dliom_front_end* fe, const dliom_cloud** high_resolution,
                                   const dliom_cloud** low_resolution);
int dliom_front_end_active_submap(const dliom_front_end* fe, int i, double local_pose[7], int* num_range_data,
                                  int* finished, dliom_grid** high_resolution_grid,
                                  dliom_grid** low_resolution_grid);
/* sensor::VoxelFilter::Filter / AdaptiveVoxelFilter::Filter (sensor/internal/voxel_filter.cc:81-90,
 * 28-77,147-150) on device-resident clouds: *out is a new cloud (dliom_cloud_destroy) holding the
 * survivors in input order -- the first point of every voxel lround(p / size).  Bit-identical to
 * the host filters below for |p / size| < 2^20 per axis, DLIOM_ERR_INVALID_ARGUMENT beyond. */
int dliom_cloud_voxel_filter(dliom_ctx* ctx, const dliom_cloud* in, float size, dliom_cloud** out);
int dliom_cloud_adaptive_voxel_filter(dliom_ctx* ctx, const dliom_cloud* in,
                                      const dliom_adaptive_voxel_filter_options* options, dliom_cloud** out);
/* The two AdaptiveVoxelFilter::Filter calls of LocalTrajectoryBuilder3D::AddAccumulatedRangeData
 * (local_trajectory_builder_3d.cc:507-512 high resolution, :523-533 low resolution) on the same cloud, searched
 * together: each result equals dliom_cloud_adaptive_voxel_filter() with that option set, for the launch and
 * readback round trips of one call. */
int dliom_cloud_adaptive_voxel_filter_pair(dliom_ctx* ctx, const dliom_cloud* in,
                                           const dliom_adaptive_voxel_filter_options* first,
                                           const dliom_adaptive_voxel_filter_options* second, dliom_cloud** out_first,
                                           dliom_cloud** out_second);
/* The approximate voxel grid: pcl::ApproximateVoxelGrid<PointXYZ> as PCL 1.8.0 runs it, on a device-resident cloud
 * (LocalTrajectoryBuilder3D::MatchByNDT, local_trajectory_builder_3d.cc:969-1008, filters both of its clouds with it at
 * 0.2 m).  THE DEFINITION, float arithmetic, every operation rounded on its own:
 *   inv = 1.0f / leaf.  A point's voxel is (floor(x * inv), floor(y * inv), floor(z * inv)) in float, cast to int; its slot
 *   is (ix * 7171 + iy * 3079 + iz * 4231) & 511 in wrapping 32-bit arithmetic.  The points are taken in input order into a
 *   table of 512 slots.  A slot that holds another voxel is flushed to the output first (centroid = float sums / (float)count,
 *   the sums taken from +0.0 in input order) and starts anew; at the end the occupied slots are flushed in slot order.
 * *out is a new cloud that equals that loop bit for bit, in values and in order (the adapter's host class
 * registration::ApproximateVoxelGrid is the loop itself).  The output depends on the input order, but only within a slot:
 * the device replays the 512 slots as independent streams.  xyz only.  An empty input gives an empty cloud.
 * DLIOM_ERR_INVALID_ARGUMENT: NULLs, a cloud of another context, leaf <= 0 or NaN, a non-finite coordinate, a floor(p * inv)
 * outside [-2^31, 2^31) (the cast is undefined there).  One read-back a call. */
int dliom_cloud_approximate_voxel_filter(dliom_ctx* ctx, const dliom_cloud* in, float leaf, dliom_cloud** out);
/* The points of a cloud in input order, packed xyz (room for dliom_cloud_size points). */
int dliom_cloud_download(const dliom_cloud* cloud, float* points_xyz);
/* ... moved by a float pose [tx, ty, tz, qw, qx, qy, qz]: sensor::TransformPointCloud(cloud, pose) (sensor/point_cloud.cc:25-33,
 * rotation * p + translation in Eigen's operation order) -- LocalTrajectoryBuilder3D's
 * filtered_range_data_in_local = TransformRangeData(filtered_range_data_in_tracking, opt_pose.cast<float>())
 * (local_trajectory_builder_3d.cc:556-559) without a host loop over the returns. */
int dliom_cloud_download_transformed(const dliom_cloud* cloud, const float pose[7], float* points_xyz);

/* ---- Point-cloud export: the points-processor stages with compute in them (cartographer/io) ----
 * io::OutlierRemovingPointsProcessor (io/outlier_removing_points_processor.{h,cc}, the pipeline action
 * "voxel_filter_and_remove_moving_objects") streams every batch of a trajectory three times over a
 * HybridGridBase<VoxelData {int hits; int rays;}> (.h:55-58, 81): mark hits, count the rays through voxels that have
 * hits, drop the points of voxels with rays >= 3 * hits.  A dliom_outlier_remover is that grid as a sparse voxel table
 * in HBM; every count equals the reference's (integers only: no result depends on the order of the device's atomics).
 * Clouds hold map-frame points, like io::PointsBatch::points; the caller supplies the batch origin.
 *
 * Where the reference aborts, hangs or is undefined, a call returns an error and leaves the table as it was:
 *   DLIOM_ERR_GRID_EXTENT       mark_hits: a hit whose cell index leaves [-8192, 8191] on an axis (Grow()'s
 *                               CHECK_LE(new_bits, 8), hybrid_grid.h:389)
 *   DLIOM_ERR_INVALID_ARGUMENT  a non-finite coordinate or origin (lround of it is undefined); a call out of phase order
 *   DLIOM_ERR_RAY_TOO_LONG      count_rays: a ray of voxel_size * 2^24 or more (`x += voxel_size_` stops advancing in
 *                               float and the reference's loop does not end, .cc:98)
 * A pass-2 sample or a pass-3 point outside the extent reads ValueType() as in the reference (value(),
 * hybrid_grid.h:266-271): nothing is counted, and pass 3 removes the point (!(0 < 0)).
 * Phases are one-way like the reference's State (.h:59-63): mark_hits after the first successful count_rays, or
 * count_rays after the first successful filter, is refused.
 * NULL pointers, a voxel_size that is not finite and positive (as double and as float) and a negative capacity are
 * refused with DLIOM_ERR_INVALID_ARGUMENT before anything touches a device.
 * Every call runs on the context's stream and has finished with its inputs when it returns: mark_hits and count_rays
 * read back only their error flag (mark_hits with it the number of leaves, which sizes the pool), filter the survivor
 * count.  The table grows between launches, never inside a kernel. */
typedef struct dliom_outlier_remover dliom_outlier_remover;
typedef struct dliom_outlier_stats {
  int64_t voxels;          /* voxels with hits > 0 */
  int64_t leaves;          /* 8x8x8 blocks of voxels in use (4 KiB each) */
  int64_t leaf_capacity, table_capacity; /* allocated leaves; entries of the leaf hash table */
  int64_t table_bytes;     /* HBM held: hash table, leaf pool, counters */
  int64_t growths;         /* reallocations of the hash table or the pool since creation */
  int64_t samples_walked;  /* pass-2 samples so far (iterations of the loop at .cc:98) */
  int64_t probes;          /* hash-table entries read by pass 2 so far */
  int phase;               /* 1, 2, 3 */
} dliom_outlier_stats;
/* OutlierRemovingPointsProcessor(voxel_size, next) (.cc:36-43): the grid's resolution is float(voxel_size), the ray step
 * stays double. */
int dliom_outlier_remover_create(dliom_ctx* ctx, double voxel_size, dliom_outlier_remover** out);
int dliom_outlier_remover_destroy(dliom_outlier_remover* remover);
/* ProcessInPhaseOne (.cc:84-90): ++hits in the voxel of every point. */
int dliom_outlier_remover_mark_hits(dliom_outlier_remover* remover, const dliom_cloud* points);
/* ProcessInPhaseTwo (.cc:92-108): for every point, for (float x = 0; x < length; x += voxel_size), ++rays in the voxel
 * of origin + (x / length) * delta if it has hits.  Two samples of a ray in one voxel count twice. */
int dliom_outlier_remover_count_rays(dliom_outlier_remover* remover, const float origin[3], const dliom_cloud* points);
/* ProcessInPhaseThree (.cc:110-124) with RemovePoints (points_batch.cc:22-49): *kept = the points whose voxel has
 * rays < 3 * hits, in input order (a new cloud, the caller destroys it); kept_index (may be NULL; capacity entries)
 * receives their input indices, for the caller's intensities and colors.  *num_kept is always filled; a kept_index
 * too small for it returns DLIOM_ERR_CAPACITY and no cloud. */
int dliom_outlier_remover_filter(dliom_outlier_remover* remover, const dliom_cloud* points, dliom_cloud** kept,
                                 int32_t* kept_index, int64_t capacity, int64_t* num_kept);
/* The table (the reference's voxels_, .h:81): every voxel with hits > 0, sorted by (z, y, x); xyz 3 * capacity ints,
 * hits and rays capacity ints.  All three NULL: *count only.  Too small a capacity: *count and DLIOM_ERR_CAPACITY. */
int dliom_outlier_remover_voxels(const dliom_outlier_remover* remover, int32_t* xyz, int32_t* hits, int32_t* rays,
                                 int64_t capacity, int64_t* count);
int dliom_outlier_remover_stats(const dliom_outlier_remover* remover, dliom_outlier_stats* out);
/* MinMaxRangeFiteringPointsProcessor::Process (io/min_max_range_filtering_points_processor.cc:40-51): keeps the points
 * with min_range <= range && range <= max_range, range = (p - origin).norm() in float, the bounds in double; order kept.
 * kept_index, capacity, num_kept as in dliom_outlier_remover_filter.  NaN bounds are refused. */
int dliom_cloud_min_max_range_filter(dliom_ctx* ctx, const dliom_cloud* in, const float origin[3], double min_range,
                                     double max_range, dliom_cloud** out, int32_t* kept_index, int64_t capacity,
                                     int64_t* num_kept);
/* ---- The head of the export: batches assembled from sensor-frame points (cartographer_ros/assets_writer.cc:119-160) ----
 * transform::TransformInterpolationBuffer (transform/transform_interpolation_buffer.{h,cc}) as an immutable array of
 * nodes: times in common::Time ticks (100 ns), poses [tx,ty,tz,qw,qx,qy,qz] of tracking in map.  Decreasing times are
 * refused with DLIOM_ERR_INVALID_ARGUMENT (Push's CHECK_GE); equal neighbours are allowed; n = 0 is the empty buffer.
 * ctx may be NULL: a host-only buffer for dliom_trajectory_lookup (dliom_cloud_from_sensor_points refuses it).  The nodes
 * reach the device with the first call that needs them there.  A trajectory may be destroyed after its context (it then
 * only frees its own device memory); it may not be used after it. */
typedef struct dliom_trajectory dliom_trajectory;
int dliom_trajectory_create(dliom_ctx* ctx, const int64_t* times, const double* poses7, int64_t n, dliom_trajectory** out);
int dliom_trajectory_destroy(dliom_trajectory* trajectory);
int dliom_trajectory_size(const dliom_trajectory* trajectory, int64_t* n);
/* Has(time) and, where it holds and pose7 is not NULL, Lookup(time) (host only): the node's own transform when
 * lower_bound's node has that time, else Interpolate(prev, node) (transform/timestamped_transform.cc:22-37: translations
 * blended in double, Eigen's slerp with its 1 - epsilon threshold and sign flip, not renormalised). */
int dliom_trajectory_lookup(const dliom_trajectory* trajectory, int64_t time, int* has, double pose7[7]);
/* HandleMessage's loop over the n points (x, y, z, relative time [s]) of one message in the sensor frame.  Point i has
 * time = cloud_time + int64(double(t_i) * 1e7) (common::FromSeconds); it is dropped unless the trajectory Has(time), else
 * transformed in float by (Lookup(time) * sensor_to_tracking).cast<float>().  *out: the kept points in input order (a new
 * cloud, the caller destroys it), NULL with status OK when none is kept (the reference returns nullptr).  origin: the
 * translation of the last kept point's transform.  kept_index, capacity, num_kept as in dliom_outlier_remover_filter.
 * The floats are the reference's, proven per call (dliom_assemble_check_stats).  DLIOM_ERR_INVALID_ARGUMENT, before
 * anything is written: a t_i that is not finite or has |t_i * 1e7| >= 2^63, NULL arguments, a trajectory of another
 * context, negative n.  Coordinates are not checked: non-finite ones are passed through, as the reference does. */
int dliom_cloud_from_sensor_points(dliom_ctx* ctx, dliom_trajectory* trajectory, int64_t cloud_time, const float* points_xyzt,
                                   int64_t n, const double sensor_to_tracking[7], dliom_cloud** out, float origin[3],
                                   int32_t* kept_index, int64_t capacity, int64_t* num_kept);
/* The check behind it: points whose casts to float the device could not prove equal to glibc's (recorded), records the
 * host recomputed with glibc, points it had to redo, and calls whose records outgrew the words read back anyway. */
int dliom_assemble_check_stats(const dliom_ctx* ctx, int64_t* recorded, int64_t* recomputed, int64_t* fixed, int64_t* ring_overflows);
/* The same filters on host buffers (the reference's own placement): out_xyz has room for n points;
 * *num_out receives the survivors (first point per voxel). */
int dliom_voxel_filter(float size, const float* points_xyz, int64_t n, float* out_xyz, int64_t* num_out);
int dliom_adaptive_voxel_filter(const dliom_adaptive_voxel_filter_options* options, const float* points_xyz,
                                int64_t n, float* out_xyz, int64_t* num_out);

/* ---- X-ray images of point clouds (the pipeline action "write_xray_image") ----
 * io::XRayPointsProcessor (io/xray_points_processor.{h,cc}) projects every batch through a Rigid3f into a
 * HybridGridBase<bool> of occupied voxels and a std::map<(y, z), ColumnData {float sum_r, sum_g, sum_b; uint32 count}>
 * (.h:61-71), and at Flush paints one pixel per column (y, z): its mean colour, saturated by the logarithm of the
 * number of occupied voxels in the column.  A dliom_points_xray is one such Aggregation in HBM.  Voxels, counts and the
 * bounding box are integers; the colour sums are the reference's sequential float sums in point order, batch after
 * batch, bit for bit -- so the tables and the image equal the reference's exactly.
 *
 * Where the reference aborts or is undefined, insert returns an error and leaves the aggregator as it was:
 *   DLIOM_ERR_GRID_EXTENT       a transformed point whose cell index leaves [-8192, 8191] (hybrid_grid.h:389)
 *   DLIOM_ERR_INVALID_ARGUMENT  a transformed point that is not finite (lround of it is undefined)
 * NULL pointers, a voxel_size that is not finite and positive (as double and as float), a non-finite transform, a
 * colour count other than 0, 1 or the number of points and a negative capacity are refused with
 * DLIOM_ERR_INVALID_ARGUMENT before anything touches a device.  Colours are not checked: non-finite colours give
 * unspecified pixels, as they do in the reference.
 * The pixels are io::Image's (image.h): 0xFF000000 | r << 16 | g << 8 | b, row-major.  PNG encoding, cairo and
 * DrawTrajectory stay with the caller. */
typedef struct dliom_points_xray dliom_points_xray;
typedef struct dliom_points_xray_statistics {
  int64_t voxels;           /* occupied voxels */
  int64_t columns;          /* slots of the column table (entries of column_data, see dliom_points_xray_columns) */
  int64_t leaves;           /* 8x8x8 blocks of voxels in use (64 bytes each) */
  int64_t table_bytes;      /* HBM held: both hash tables, leaf masks, column arrays, counters, scratch */
  int64_t probes;           /* hash-table entries read by the inserts so far */
  int64_t longest_segment;  /* most points of one batch in one column so far: the length of the longest ordered sum */
  int64_t growths;          /* reallocations of a table or a pool since creation */
  int64_t inserts, points;  /* successful non-empty inserts and their points */
} dliom_points_xray_statistics;
/* XRayPointsProcessor(voxel_size, transform, ...) (.cc:98-116), one Aggregation: HybridGridBase<bool>(voxel_size) takes
 * float(voxel_size); transform7 = [tx, ty, tz, qw, qx, qy, qz] of transform_. */
int dliom_points_xray_create(dliom_ctx* ctx, double voxel_size, const float transform7[7], dliom_points_xray** out);
int dliom_points_xray_destroy(dliom_points_xray* xray);
/* Insert (.cc:195-213).  num_colors 0: batch.colors is empty, kDefaultColor black; 1: colors_rgb[0..2] for every point
 * (what ColoringPointsProcessor produces); points' size: colors_rgb holds r, g, b per point.  colors_rgb is a host
 * pointer (page-locked memory of dliom_host_register is copied from without staging) and is free when the call returns. */
int dliom_points_xray_insert(dliom_points_xray* xray, const dliom_cloud* points, const float* colors_rgb, int64_t num_colors);
/* bounding_box_ (.cc:203) of this aggregator's inserts: cell indices; *empty as AlignedBox3i::isEmpty (min, max then
 * hold INT32_MAX, INT32_MIN).  The reference keeps one box for all floors: the caller merges. */
int dliom_points_xray_bounding_box(const dliom_points_xray* xray, int32_t box_min[3], int32_t box_max[3], int* empty);
/* column_data, sorted by (y, z) like the std::map: yz 2 * capacity ints, sums_rgb 3 * capacity floats, counts and
 * occupied (the number of occupied voxels of the column, .cc:174) capacity each.  All four NULL: *count only.  Too small
 * a capacity: *count and DLIOM_ERR_CAPACITY.  (An insert that fails with DLIOM_ERR_HIP while its pools grow -- out of
 * memory -- inserts none of its points; the column keys it had claimed hold no points and are not listed.) */
int dliom_points_xray_columns(const dliom_points_xray* xray, int32_t* yz, float* sums_rgb, uint32_t* counts, uint32_t* occupied,
                              int64_t capacity, int64_t* count);
/* The occupied voxels (aggregation.voxels, .cc:164), sorted by (z, y, x); xyz 3 * capacity ints, NULL: *count only. */
int dliom_points_xray_voxels(const dliom_points_xray* xray, int32_t* xyz, int64_t capacity, int64_t* count);
/* WriteVoxels + IntoImage (.cc:46-84, 144-175) in the box [box_min, box_max] of cell indices (both NULL: the
 * aggregator's own): width = sizes[1] + 1, height = sizes[2] + 1, pixel (box_max[1] - y, box_max[2] - z).  *width and
 * *height are always filled; argb NULL: sizes only; capacity (pixels) too small: DLIOM_ERR_CAPACITY.  An empty box gives
 * DLIOM_OK and width = height = 0 ("Not writing output", .cc:146-149).  A box that does not hold every voxel of the
 * aggregator is refused (the reference would write outside its matrix). */
int dliom_points_xray_draw(const dliom_points_xray* xray, const int32_t box_min[3], const int32_t box_max[3], uint32_t* argb,
                           int64_t capacity, int32_t* width, int32_t* height);
int dliom_points_xray_stats(const dliom_points_xray* xray, dliom_points_xray_statistics* out);
/* One pixel of IntoImage on the host (.cc:64-81, io/color.h:35-38): a column of `occupied` voxels in an image whose
 * fullest column has max_occupied, with the column's mean colour.  occupied == 0: white.  What the device paints. */
int dliom_points_xray_pixel(uint32_t occupied, uint32_t max_occupied, const float mean_rgb[3], uint32_t* argb);

/* ---- Export batches in HBM: io::PointsBatch with its intensities and colours on the device (cartographer/io) ----
 * A dliom_points_batch owns one dliom_cloud of map-frame points, the origin (host), and optionally one intensity and one
 * colour (r, g, b) a point, all in HBM.  The stages below read and rewrite it where it is: every compacting stage is
 * RemovePoints (io/points_batch.cc:22-49) on the three vectors at once, and reads back the kept count and nothing else.
 * Attribute counts are 0 or the number of points, as RemovePoints assumes (:40-45 index past the end otherwise); an
 * empty batch has neither attribute, like the reference's empty vectors.
 *
 * NULL pointers, a count that is negative or neither 0 nor n, NaN bounds and an object of another context are refused
 * with DLIOM_ERR_INVALID_ARGUMENT before anything touches a device.  A failed call leaves the batch as it was.
 * Blocks go back to the cloud pool like a cloud's, each after a whole-device synchronise (not counted by
 * dliom_ctx_synchronizations): a compacting call gives back up to three (cloud, intensities, colours), dliom_points_batch_color
 * one when the batch held a colour a point. */
typedef struct dliom_points_batch dliom_points_batch;
/* points_xyz: n points; origin: 3 floats; intensities: n floats or NULL; colors_rgb: num_colors * 3 floats, num_colors 0
 * (colors_rgb may be NULL) or n.  Host pointers, free when the call returns. */
int dliom_points_batch_create(dliom_ctx* ctx, const float* points_xyz, int64_t n, const float origin[3], const float* intensities,
                              const float* colors_rgb, int64_t num_colors, dliom_points_batch** out);
int dliom_points_batch_destroy(dliom_points_batch* batch);
int dliom_points_batch_size(const dliom_points_batch* batch, int64_t* n);
int dliom_points_batch_has_intensities(const dliom_points_batch* batch, int* has);
int dliom_points_batch_has_colors(const dliom_points_batch* batch, int* has);
/* The batch's points, borrowed: valid until the next call that compacts or destroys the batch.  What
 * dliom_outlier_remover_mark_hits / _count_rays, dliom_inserter2d_insert_cloud and dliom_inserter_insert_cloud take. */
int dliom_points_batch_cloud(const dliom_points_batch* batch, const dliom_cloud** cloud);
int dliom_points_batch_origin(const dliom_points_batch* batch, float origin[3]);
/* points_xyz 3 n floats, intensities n, colors_rgb 3 n; any of them may be NULL.  A requested attribute the batch does
 * not have is refused. */
int dliom_points_batch_download(const dliom_points_batch* batch, float* points_xyz, float* intensities, float* colors_rgb);
/* dliom_cloud_from_sensor_points with the kept points' intensities (n floats or NULL) gathered on the device in the same
 * call: the message's intensities are uploaded once and never come back.  *out is NULL with DLIOM_OK when nothing is
 * kept.  Refusals and the per-call exactness check are dliom_cloud_from_sensor_points' own. */
int dliom_points_batch_from_sensor_points(dliom_ctx* ctx, dliom_trajectory* trajectory, int64_t cloud_time, const float* points_xyzt,
                                          const float* intensities, int64_t n, const double sensor_to_tracking[7],
                                          dliom_points_batch** out);
/* dliom_cloud_min_max_range_filter about the batch's origin, in place. */
int dliom_points_batch_min_max_range_filter(dliom_points_batch* batch, double min_range, double max_range);
/* dliom_outlier_remover_filter (phase three), in place. */
int dliom_outlier_remover_filter_batch(dliom_outlier_remover* remover, dliom_points_batch* batch);
/* ColoringPointsProcessor::Process (io/coloring_points_processor.cc:45-53): every point gets rgb.  (The frame_id
 * comparison is the caller's.) */
int dliom_points_batch_color(dliom_points_batch* batch, const float rgb[3]);
/* IntensityToColorPointsProcessor::Process (io/intensity_to_color_points_processor.cc:47-58): gray =
 * Clamp((intensity - min) / (max - min), 0.f, 1.f) in float with IEEE division; common::Clamp (common/math.h:32-40) lets
 * NaN through, and max == min gives the host's infinities and NaNs.  A batch without intensities is left alone. */
int dliom_points_batch_intensity_to_color(dliom_points_batch* batch, float min_intensity, float max_intensity);
/* dliom_points_xray_insert with the batch's colours read where they are (none: black; one for the batch; one a point).
 * A batch of ONE point with a per-point colour reads those 12 bytes back first (one stream synchronise): the insert's
 * single-colour path takes its colour from the host, as it does for the host entry. */
int dliom_points_xray_insert_batch(dliom_points_xray* xray, const dliom_points_batch* batch);

/* common::FixedRatioSampler (common/fixed_ratio_sampler.cc:32-39) behind io::FixedRatioSamplingPointsProcessor
 * (io/fixed_ratio_sampling_points_processor.cc:43-53): per point, ++num_pulses; kept iff
 * double(num_samples) / num_pulses < ratio, then ++num_samples.  Both counters are int64 and run on from batch to batch.
 * The device runs chunks of consecutive pulses from guessed starting counts, proves every chunk's start against its
 * predecessor's end, and re-runs the chunks whose start was wrong until none is: the result is the sequential loop's,
 * whatever the guess.  A ratio outside [0, 1] or NaN is refused (CHECK_GE / CHECK_LE). */
typedef struct dliom_fixed_ratio_sampler dliom_fixed_ratio_sampler;
typedef struct dliom_fixed_ratio_sampler_statistics {
  int64_t chunks;          /* chunks run so far, first passes only */
  int64_t repaired_chunks; /* chunks re-run because their guessed start was wrong */
  int64_t repair_passes;   /* passes after the first, over all calls */
} dliom_fixed_ratio_sampler_statistics;
int dliom_fixed_ratio_sampler_create(double ratio, dliom_fixed_ratio_sampler** out);
int dliom_fixed_ratio_sampler_destroy(dliom_fixed_ratio_sampler* sampler);
/* (0, 0) again: what Flush does when the stream restarts. */
int dliom_fixed_ratio_sampler_reset(dliom_fixed_ratio_sampler* sampler);
int dliom_fixed_ratio_sampler_state(const dliom_fixed_ratio_sampler* sampler, int64_t* num_pulses, int64_t* num_samples);
int dliom_fixed_ratio_sampler_stats(const dliom_fixed_ratio_sampler* sampler, dliom_fixed_ratio_sampler_statistics* out);
/* One Pulse() a point, in order; the batch is compacted in place and the state advances by its size.  One read-back a
 * pass (kept count and the number of wrong starts together). */
int dliom_points_batch_fixed_ratio_sample(dliom_fixed_ratio_sampler* sampler, dliom_points_batch* batch);

/* The writers' per-point loops (io/ply_writing_points_processor.cc:138-147, io/pcd_writing_points_processor.cc:121-128)
 * as packed records, built on the device and downloaded in one copy.
 *   PLY: x y z (little-endian floats) [r g b bytes: ToUint8Color] [intensity float]       12, 15, 16 or 19 bytes
 *   PCD: x y z [b g r 0 bytes]                                                         12 or 16 bytes
 * ToUint8Color (io/color.h:35-45) is uint8(lround(Clamp(c, 0.f, 1.f) * 255)): a float product rounded half away from
 * zero; infinite components clamp; a NaN component gives an unspecified byte, as lround does in the reference.
 * with_colors / with_intensities are the FILE's layout, decided by the writer at its first non-empty batch; a non-empty
 * batch that lacks an attribute the file has is refused (the reference's CHECK_EQ).  PCD never writes intensities
 * (with_intensities must be 0) and takes its colours from the batch: with_colors must equal the batch's own.
 * *num_bytes is always filled; bytes NULL: the size only; capacity < *num_bytes: DLIOM_ERR_CAPACITY.  Exactly *num_bytes
 * bytes are written. */
#define DLIOM_PACK_PLY 0
#define DLIOM_PACK_PCD 1
int dliom_points_batch_pack(const dliom_points_batch* batch, int format, int with_colors, int with_intensities, uint8_t* bytes,
                            int64_t capacity, int64_t* num_bytes);
/* WriteBinaryPlyHeader (.cc:35-56) and WriteBinaryPcdHeader (.cc:35-57), byte for byte (host only): the count is
 * zero-padded to 15 digits, so the placeholder written with count 0 and the final header have one length.  buffer,
 * capacity, *length as dliom_ros_map_pgm_header.  A negative count is refused. */
int dliom_ply_header(int with_colors, int with_intensities, int64_t num_points, char* buffer, int64_t capacity, int64_t* length);
int dliom_pcd_header(int with_colors, int64_t num_points, char* buffer, int64_t capacity, int64_t* length);

/* ---- XYZ text of export batches (the pipeline action "write_xyz"; io/xyz_writing_points_processor.cc:13-20) ----
 * Text of a float.  What `std::ostream << std::setprecision(6) << float` writes under glibc / libstdc++, which is
 * printf("%.6g") of the value promoted to double; at most 12 characters ("-0.000123456", "-1.17549e-38").
 *   zero       "0", and "-0" with the sign bit set
 *   infinity   "inf", "-inf"
 *   NaN        "nan", and "-nan" with the sign bit set (the payload does not show)
 *   otherwise  an optional '-', then the six significant decimal digits D (10^5 <= D < 10^6) and the decimal exponent X
 *              of the float's EXACT value v: D = v / 10^(X - 5) rounded to the nearest integer, a tie to the even one --
 *              so 1000.125f is "1000.12", 1.015625f "1.01562", 100000.5f "100000" and 100001.5f "100002".  A D that
 *              rounds up to 10^6 is 10^5 with X one larger (999999.5f is "1e+06").
 *              -4 <= X < 6: fixed notation, the decimal point behind digit X (in front of -X - 1 zeros and "0." for
 *              X < 0), trailing zeros of the fraction and a bare '.' removed ("100", "0.0001", "2.5").
 *              else: d[.ddddd]e+XX or e-XX, trailing zeros and a bare '.' removed, two exponent digits ("1e+06",
 *              "1.17549e-38"; |X| <= 45).
 * The device and dliom_float_text run ONE integer-only formatter (csrc/float_text.h): no floating-point rounding decides
 * a digit, and the device's bytes equal the host's for every bit pattern.  No locale: the point is '.'.
 *
 * Record of a point.  x, ' ', y, ' ', z, '\n': 6 to DLIOM_XYZ_MAX_RECORD bytes.  Intensities and colours are ignored, as
 * the reference ignores them, and nothing about the batch changes.
 *
 * dliom_points_batch_pack_xyz / dliom_cloud_pack_xyz follow dliom_points_batch_pack's conventions: *num_bytes is always
 * the exact size of the text; bytes NULL: the size only (one read-back); capacity < *num_bytes: DLIOM_ERR_CAPACITY and
 * nothing written; else exactly *num_bytes bytes are written (two host synchronisations: the size, then the download).
 * An empty batch gives DLIOM_OK and 0 bytes without touching the device.  capacity >= DLIOM_XYZ_MAX_RECORD * n NEVER
 * returns DLIOM_ERR_CAPACITY: a caller that brings such a buffer needs one call only.  Byte offsets into the text are
 * 64-bit on the host and on the device, so no size a batch can have (n <= 2^31 - 1) wraps; the scratch holds
 * min(capacity, DLIOM_XYZ_MAX_RECORD * n) bytes of text, and a batch too large for the device's memory fails with
 * DLIOM_ERR_HIP.  NULL batch / cloud / num_bytes and a negative capacity: DLIOM_ERR_INVALID_ARGUMENT. */
#define DLIOM_XYZ_MAX_RECORD 39
/* Host only.  buffer takes the characters (no terminator), *length their number (<= 12).  NULL: refused. */
int dliom_float_text(float value, char buffer[16], int32_t* length);
int dliom_points_batch_pack_xyz(const dliom_points_batch* batch, uint8_t* bytes, int64_t capacity, int64_t* num_bytes);
int dliom_cloud_pack_xyz(const dliom_cloud* cloud, uint8_t* bytes, int64_t capacity, int64_t* num_bytes);

/* ---- 2D probability grid of the export pipeline (the actions "write_probability_grid" and "write_ros_map") ----
 * io::ProbabilityGridPointsProcessor (io/probability_grid_points_processor.{h,cc}) and
 * cartographer_ros::RosMapWritingPointsProcessor (ros_map_writing_points_processor.cc:52-94, ros_map.cc:21-47) insert
 * every batch into a mapping::ProbabilityGrid with ProbabilityGridRangeDataInserter2D
 * (probability_grid_range_data_inserter_2d.cc:48-64) and draw it at the end.  A dliom_probability_grid is that grid in
 * HBM: dense uint16 correspondence-cost cells, row-major num_x_cells * y + x (grid_2d.cc:168-171); MapLimits and the
 * known-cells box live on the host.  Every cell, limit and pixel equals the reference's bit for bit (DESIGN.md
 * section 3.11): the arithmetic is double up to the cell index (map_limits.h:69-76) and integer from there on.
 *
 * Refusals leave the grid exactly as it was:
 *   DLIOM_ERR_INVALID_ARGUMENT  NULL or wrong-context arguments, negative n (before anything touches a device); a
 *                               non-finite x or y of the origin or of a point (lround of it is undefined; z is
 *                               never read, as in the reference: head<2>())
 *   DLIOM_ERR_GRID_EXTENT       growth that would need num_cells * 1000 beyond int (the superscaled CellLimits of
 *                               ray_casting.cc:175-178 overflows), a cell index that the reference's long -> int
 *                               narrowing would wrap (map_limits.h:73-75), a superscaled index outside the grid
 *                               (CHECK_GE ray_casting.cc:38-40, CHECK(Contains) grid_2d.cc:169), or more bytes of
 *                               cells than the grid's budget
 *   DLIOM_ERR_INTERNAL          the device error word is set (never expected; the passes have written: the grid is NOT
 *                               restored, the known-cells box is extended and the insert counted like any other)
 * An insert reads back twice: the batch's float bounding box with the non-finite flag (GrowAsNeeded runs on the
 * host, between launches), and after the last pass the error words -- so a call has finished with its inputs
 * when it returns. */
typedef struct dliom_probability_grid dliom_probability_grid;
typedef struct dliom_inserter2d dliom_inserter2d;
#define DLIOM_PROBABILITY_GRID_DEFAULT_BUDGET_BYTES (INT64_C(1) << 30) /* of cells: 23170 x 23170 */
typedef struct dliom_probability_grid_stats {
  int64_t bytes;          /* HBM held: cells, colour table, words */
  int64_t growths;        /* doublings since creation (grid_2d.cc:118) */
  int64_t inserts;        /* successful inserts */
  int64_t cells_visited;  /* ApplyLookupTable calls of the ray passes so far (ray_casting.cc:49,89-142) */
  int32_t known_box[4];   /* min x, min y, max x, max y (grid_2d.h known_cells_box_); min > max: empty */
  int32_t error_word;     /* the device error word as last read */
} dliom_probability_grid_stats;
/* io::CreateProbabilityGrid (probability_grid_points_processor.cc:150-158): 100 x 100 cells, max = 0.5 * 100 *
 * resolution on both axes.  budget_bytes <= 0: DLIOM_PROBABILITY_GRID_DEFAULT_BUDGET_BYTES. */
int dliom_probability_grid_create(dliom_ctx* ctx, double resolution, int64_t budget_bytes, dliom_probability_grid** out);
/* ProbabilityGrid(MapLimits(resolution, (max_x, max_y), CellLimits(num_x_cells, num_y_cells))), e.g. the fixture of
 * range_data_inserter_2d_test.cc:35. */
int dliom_probability_grid_create_with_limits(dliom_ctx* ctx, double resolution, double max_x, double max_y,
                                              int32_t num_x_cells, int32_t num_y_cells, int64_t budget_bytes,
                                              dliom_probability_grid** out);
int dliom_probability_grid_destroy(dliom_probability_grid* grid);
/* limits(): resolution, max (x, y), cell limits (x, y) (map_limits.h:44-58) */
int dliom_probability_grid_limits(const dliom_probability_grid* grid, double* resolution, double max_xy[2],
                                  int32_t num_cells[2]);
/* probability_grid_bytes alone; `grids` counts HybridGrids and stays 0. */
int dliom_probability_grid_memory_stats(const dliom_probability_grid* grid, dliom_memory_stats* out);
int dliom_probability_grid_get_stats(const dliom_probability_grid* grid, dliom_probability_grid_stats* out);
/* Grid2D::GrowLimits on the limits alone (grid_2d.cc:116-145; host only, no device): grows max_xy / num_cells until
 * they contain (px, py); offset accumulates where the old cell (0, 0) lands, *doublings counts the loop's turns.
 * DLIOM_ERR_GRID_EXTENT (limits untouched) as above, with budget_bytes (<= 0: the default) on 2 bytes a cell. */
int dliom_probability_grid_grow_limits(double resolution, double max_xy[2], int32_t num_cells[2], float px, float py,
                                       int64_t budget_bytes, int32_t offset[2], int32_t* doublings);
/* ComputeLookupTableToApplyCorrespondenceCostOdds (probability_values.cc:85-101): 32768 entries. */
int dliom_compute_lookup_table_to_apply_correspondence_cost_odds(float odds, uint16_t* table);
/* ProbabilityGridRangeDataInserter2D (probability_grid_range_data_inserter_2d.cc:36-46): the two tables of
 * Odds(hit_probability), Odds(miss_probability), uploaded once.  hit_probability <= 0.5 or miss_probability >= 0.5 is
 * refused (:43-44 of the options' CHECKs). */
int dliom_inserter2d_create(dliom_ctx* ctx, double hit_probability, double miss_probability, int insert_free_space,
                            dliom_inserter2d** out);
int dliom_inserter2d_destroy(dliom_inserter2d* inserter);
/* hit_table / miss_table: 32768 entries each, read back from the device. */
int dliom_inserter2d_tables(const dliom_inserter2d* inserter, uint16_t* hit_table, uint16_t* miss_table);
/* One Insert({origin, points, {}}, grid) (:48-64 -> CastRays, ray_casting.cc:166-203): GrowAsNeeded, the hit table on
 * every end pixel, one CastRay(begin, end) per point if insert_free_space, FinishUpdate.  Map-frame points. */
int dliom_inserter2d_insert_cloud(dliom_inserter2d* inserter, dliom_probability_grid* grid, const float origin[3],
                                  const dliom_cloud* points);
int dliom_inserter2d_insert(dliom_inserter2d* inserter, dliom_probability_grid* grid, const float origin[3],
                            const float* points_xyz, int64_t n);
/* The cells: cropped = 0 the whole grid (offset 0, num_cells = the limits'), else ComputeCroppedLimits
 * (grid_2d.cc:101-111; empty box: offset 0, 1 x 1).  offset / num_cells are always filled; cells may be NULL (sizes
 * only), a capacity (in cells) below num_cells[0] * num_cells[1] returns DLIOM_ERR_CAPACITY. */
int dliom_probability_grid_cells(const dliom_probability_grid* grid, uint16_t* cells, int64_t capacity, int32_t offset[2],
                                 int32_t num_cells[2], int cropped);
/* GetProbability / IsKnown (probability_grid.cc:69-73, grid_2d.cc:93-97) of n cells (x, y); outside the limits:
 * kMinProbability, unknown.  known may be NULL. */
int dliom_probability_grid_get_probabilities(const dliom_probability_grid* grid, const int32_t* cell_xy, int64_t n,
                                             float* probabilities, uint8_t* known);
/* DrawProbabilityGrid (probability_grid_points_processor.cc:127-148) on the device: one gray byte a pixel of the
 * cropped box, 128 unknown, else ProbabilityToColor (:49-54).  rotate_cw = 1 also applies
 * Image::Rotate90DegreesClockwise (io/image.cc:67-76): size = {height, width} of the unrotated image.  offset / size
 * are filled; gray may be NULL (sizes only); too small a capacity returns DLIOM_ERR_CAPACITY.  There is always an image:
 * DrawProbabilityGrid returns nullptr only for cropped limits with a zero side (:131-134), and ComputeCroppedLimits
 * gives 1 x 1 for an empty box (grid_2d.cc:103-107), so a fresh grid draws one unknown pixel, as in the reference. */
int dliom_probability_grid_draw(const dliom_probability_grid* grid, uint8_t* gray, int64_t capacity, int32_t offset[2],
                                int32_t size[2], int rotate_cw);
/* The 32768 gray values draw uses (host only). */
int dliom_probability_grid_color_table(uint8_t* table);
/* The YAML origin of ros_map_writing_points_processor.cc:73-76 with the ROTATED image's width / height (host only). */
int dliom_ros_map_yaml_origin(double resolution, const double max_xy[2], const int32_t offset[2], int32_t width,
                              int32_t height, double origin[2]);
/* WritePgm's header (ros_map.cc:23-26) and WriteYaml's text (:41-45) into buffer (capacity bytes, no terminator);
 * *length is always filled, DLIOM_ERR_CAPACITY if it does not fit (host only). */
int dliom_ros_map_pgm_header(double resolution, int32_t width, int32_t height, char* buffer, int64_t capacity,
                             int64_t* length);
int dliom_ros_map_yaml(double resolution, const double origin[2], const char* pgm_filename, char* buffer,
                       int64_t capacity, int64_t* length);

/* ---- per-hit de-skew of LocalTrajectoryBuilder3D::AddRangeData -------------------------------
 * (mapping/internal/3d/local_trajectory_builder_3d.cc:421-472, InterpolatePose :869-877).
 * hits_xyzt: n x (x, y, z, t) in the tracking frame, t <= 0 seconds relative to the scan end (the
 * hits that survived VoxelFilter(0.5 * voxel_filter_size), :393-395).  For every hit: s = (T + t)/T,
 * pose_i = (prev_pose * [s t_rel, slerp(I, q_rel, s)]).cast<float>() with rel = prev^-1 * predicted,
 * hit and origin moved into the local frame, then the range gate: out_kind 0 = dropped
 * (range < min_range), 1 = return (out_xyz = hit_in_local), 2 = miss (out_xyz = ray cropped at
 * max_range).  If |t_0| < 1e-3 every hit takes the predicted pose ("not de-skewing", :429-433).
 * current_pose (float, [t,q]) = the last hit's pose (:477).  Slerp coefficients use the device's
 * double-precision sin/acos, which may differ from glibc's in the last ulp of a DOUBLE; the per-hit pose is cast to
 * float right after (:446).  Every hit whose cast could change under that difference is re-examined on the host with
 * glibc (dliom_deskew_check_stats below): the floats are the reference's by proof, per call. */
int dliom_deskew(dliom_ctx* ctx, const double prev_pose[7], const double predicted_pose[7], double scan_period,
                 const float* hits_xyzt, int64_t n, const float origin[3], float min_range, float max_range,
                 float* out_xyz, uint8_t* out_kind, float current_pose[7]);
/* The de-skew's float casts are PROVEN equal to the reference's, not sampled: the per-hit pose is computed in double with
 * the device's sin / acos, which may differ from glibc's in the last bits; a hit whose cast to float could change under
 * that difference (a bound derived from the libraries' documented errors, preprocess.hip) is recorded, recomputed on the
 * host with glibc -- the reference's own arithmetic -- and, should the floats differ, redone with the host's value.
 * *records_checked: hits re-examined on the host so far on this context; *ring_overflows: launches with more records
 * than ride along in the regular read-back (a second pass collects them); *hits_fixed: hits whose device cast differed
 * from glibc's (none has ever been observed). */
int dliom_deskew_check_stats(const dliom_ctx* ctx, int64_t* records_checked, int64_t* ring_overflows, int64_t* hits_fixed);

/* The whole pre-processing chain of AddRangeData on the device (:393-487), one scan per call
 * (num_accumulated_range_data = 1): ranges_xyzt (host, n x (x,y,z,t)) -> VoxelFilter(0.5 *
 * voxel_filter_size) -> de-skew + range gate as in dliom_deskew -> returns only (the 3D inserter
 * never reads RangeData::misses) -> VoxelFilter(voxel_filter_size) -> TransformRangeData by
 * current_pose.inverse().  *returns_in_tracking is a new device cloud (dliom_cloud_destroy), ready
 * for dliom_front_end_match_cloud; origin_in_tracking / current_pose as the reference computes them. */
int dliom_add_range_data(dliom_ctx* ctx, const double prev_pose[7], const double predicted_pose[7],
                         double scan_period, const float* ranges_xyzt, int64_t n, const float origin[3],
                         float min_range, float max_range, float voxel_filter_size,
                         dliom_cloud** returns_in_tracking, float origin_in_tracking[3], float current_pose[7]);
/* num_accumulated_range_data > 1 (local_trajectory_builder_3d.cc:449-476) and the RangeDataSynchronizer's two-lidar
 * output (internal/3d/range_data_synchronizer.cc:29-130): _add is one AddRangeData call up to the accumulation -- the
 * returns are de-skewed into the local frame and appended; origin_index (one float per range, NULL = all 0) selects
 * the sensor origin of `origins` (num_origins x 3, <= 4) a hit is gated against.  _finish is the tail
 * (VoxelFilter(size) over everything accumulated, TransformRangeData by the LAST current_pose^-1) and resets. */
typedef struct dliom_range_accumulator dliom_range_accumulator;
int dliom_range_accumulator_create(dliom_ctx* ctx, dliom_range_accumulator** out);
int dliom_range_accumulator_destroy(dliom_range_accumulator* accumulator);
int dliom_range_accumulator_add(dliom_range_accumulator* accumulator, const double prev_pose[7],
                                const double predicted_pose[7], double scan_period, const float* ranges_xyzt,
                                const float* origin_index, int64_t n, const float* origins, int num_origins,
                                float min_range, float max_range, float voxel_filter_size, float current_pose[7],
                                int* num_accumulated);
int dliom_range_accumulator_finish(dliom_range_accumulator* accumulator, float voxel_filter_size,
                                   dliom_cloud** returns_in_tracking, float origin_in_tracking[3]);

/* ---- FastCorrelativeScanMatcher3D (loop closure) --------------------------------
 * mapping/internal/3d/scan_matching/fast_correlative_scan_matcher_3d.h:100-132.  The constructor's
 * `nodes` arrive as what HistogramsAtAnglesFromNodes (:114-127) extracts from them: one rotational
 * histogram and one yaw per node.  The uint8 max-pool pyramid (PrecomputationGridStack3D, :57-77) is
 * built on the device at creation from `high_resolution_grid`; both grids must outlive the matcher
 * and stay unchanged (finished submaps).  Results equal the reference's: same candidate scores
 * (integer sums), same traversal order and tie handling (host recursion with the reference's
 * std::sort calls), low-resolution score by the exact sequential float sum. */
typedef struct dliom_fast_csm dliom_fast_csm;
typedef struct dliom_fast_csm_options { /* proto/scan_matching/fast_correlative_scan_matcher_options_3d.proto */
  int branch_and_bound_depth;
  int full_resolution_depth;
  double min_rotational_score;
  double min_low_resolution_score;
  double linear_xy_search_window;
  double linear_z_search_window;
  double angular_search_window;
} dliom_fast_csm_options;
typedef struct dliom_fast_csm_node_data { /* the fields of TrajectoryNode::Data the matcher reads */
  double gravity_alignment[4];                     /* w, x, y, z */
  const float* high_resolution_points;             /* packed xyz */
  int64_t num_high_resolution_points;
  const float* low_resolution_points;
  int64_t num_low_resolution_points;
  const float* rotational_scan_matcher_histogram;  /* histogram_size floats */
} dliom_fast_csm_node_data;
typedef struct dliom_fast_csm_result { /* FastCorrelativeScanMatcher3D::Result; found == 0 <=> nullptr */
  int found;
  float score;
  double pose_estimate[7];
  float rotational_score;
  float low_resolution_score;
  int num_discrete_scans;
  int64_t num_scored_candidates; /* candidates the device scored (incl. prefetched ones) */
  int64_t num_score_launches;
} dliom_fast_csm_result;
int dliom_fast_csm_create(dliom_ctx* ctx, const dliom_grid* high_resolution_grid, const dliom_grid* low_resolution_grid,
                          const float* node_histograms, const float* node_angles, int num_nodes, int histogram_size,
                          const dliom_fast_csm_options* options, dliom_fast_csm** out);
int dliom_fast_csm_destroy(dliom_fast_csm* matcher);
/* Match (:147-165), MatchFullSubmap (:204-232), MatchWith3DofInitial (:168-201). */
int dliom_fast_csm_match(dliom_ctx* ctx, const dliom_fast_csm* matcher, const double global_node_pose[7], const double global_submap_pose[7],
                         const dliom_fast_csm_node_data* constant_data, float min_score, dliom_fast_csm_result* result);
int dliom_fast_csm_match_full_submap(dliom_ctx* ctx, const dliom_fast_csm* matcher, const double global_node_rotation[4],
                                     const double global_submap_rotation[4], const dliom_fast_csm_node_data* constant_data,
                                     float min_score, dliom_fast_csm_result* result);
int dliom_fast_csm_match_with_3dof_initial(dliom_ctx* ctx, const dliom_fast_csm* matcher, const double pose_in_submap_guess[7],
                                           const dliom_fast_csm_node_data* constant_data, float min_score,
                                           dliom_fast_csm_result* result);
/* One level of the pyramid: a dense box of dims[0]*dims[1]*dims[2] uint8 (x fastest) whose element
 * (0,0,0) is cell lo[]; everything outside is 0.  values may be NULL to query the box only. */
int dliom_fast_csm_level(const dliom_fast_csm* matcher, int depth, int32_t lo[3], int32_t dims[3], uint8_t* values,
                         int64_t capacity);

/* ---- Batched loop-closure constraints ------------------------------------------------------------
 * ConstraintBuilder3D::ComputeConstraintsBetweenSubmaps (mapping/internal/constraints/constraint_builder_3d.cc:162-200)
 * schedules one ComputeConstraint task (:202-334) per (node, matched submap) pair: a fast search
 * (MatchWith3DofInitial, or Match / MatchFullSubmap), a prune when it finds nothing, and CeresScanMatcher3D::Match of
 * the node's two clouds against the submap's two grids.  The two calls below take the whole list at once.  Every result
 * equals the single call's, bit for bit; queries may name different matchers (submaps).
 *
 * Statistics of one batch call (both calls fill it when it is not NULL). */
struct dliom_batch_stats {
  int64_t batched;             /* queries / problems served by the batched device path */
  int64_t per_query;           /* ... served by the single call's own path, for the reasons below: */
  int64_t per_query_frontier;  /*   fast search outside the device frontier's limits (> 8 192 points, > 4 096
                                    lowest-resolution candidates, depth 1 or > 16 levels) */
  int64_t per_query_one_launch;/*   Ceres problem above DLIOM_TUNE_CSM_ONE_LAUNCH_MAX points */
  int64_t without_search;      /* fast search with no candidate (empty cloud, no discrete scan) or refused with
                                  DLIOM_ERR_CAPACITY; Ceres problem refused with its single call's status */
  int64_t chunks;              /* device passes the batch was cut into (scratch and page-locked memory) */
  int64_t frontier_chains;     /* fast search: discretisation + frontier chains (one per chunk) */
  int64_t lm_launches;         /* Ceres: csm_lm_batch_kernel launches (one per chunk) */
  int64_t cache_misses;        /* fast search: scores the recursion fetched on demand after the chain */
  int64_t synchronizations;    /* host round trips of the call: stream synchronisations (dliom_ctx_synchronizations) */
  int64_t read_backs;          /*   ... and polled read-backs (dliom_ctx_read_backs) */
};

enum { DLIOM_FAST_CSM_MATCH = 0, DLIOM_FAST_CSM_MATCH_FULL_SUBMAP = 1, DLIOM_FAST_CSM_MATCH_WITH_3DOF_INITIAL = 2 };
typedef struct dliom_fast_csm_query {
  int kind;                         /* DLIOM_FAST_CSM_* */
  const dliom_fast_csm* matcher;    /* created on the context's device */
  double pose[7];                   /* Match: global_node_pose; MatchFullSubmap: global_node_rotation (w, x, y, z in
                                       [0..3]); MatchWith3DofInitial: pose_in_submap_guess */
  double submap_pose[7];            /* Match: global_submap_pose; MatchFullSubmap: global_submap_rotation in [0..3] */
  dliom_fast_csm_node_data node_data;
  int histogram_size;               /* floats of node_data's histogram: must equal the matcher's */
  float min_score;
} dliom_fast_csm_query;
/* results[i] / statuses[i] = what the single call for queries[i] returns (DLIOM_ERR_CAPACITY where run_search refuses).
 * Malformed input (NULL pointers, count < 0, an unknown kind, a matcher on another device, a histogram size that
 * differs from the matcher's, node data the single call refuses) fails the whole call with DLIOM_ERR_INVALID_ARGUMENT
 * before anything runs.  The discrete scans of all queries are made in one launch and their branch-and-bound frontiers
 * in one chain, followed by the low-resolution scores of the leaves the recursions are expected to test; the host
 * recursion then runs once per query, in query order.  Large batches are cut into chunks (results do not depend on it). */
int dliom_fast_csm_match_batch(dliom_ctx* ctx, const dliom_fast_csm_query* queries, int count,
                               dliom_fast_csm_result* results, int* statuses, dliom_batch_stats* stats);

/* RotationalScanMatcher::ComputeHistogram (rotational_scan_matcher.cc:159-170; called per inserted
 * scan, local_trajectory_builder_3d.cc:605-610) on the host: histogram_size floats.  Clouds of 8192 points and more
 * are processed on up to 8 host threads (same bits at any thread count; dliom_rotational_histogram_mt(..., forced_threads = 1, ...)
 * keeps the call on the caller's thread -- the library reads no environment variable). */
int dliom_rotational_histogram(const float* points_xyz, int64_t n, int histogram_size, float* histogram);
/* The same on the device, on a cloud that is already in HBM (the filtered cloud of the front end), fused with the
 * gravity alignment of local_trajectory_builder_3d.cc:605-610: histogram of Rigid3f::Rotation(rotation_wxyz) * point
 * (rotation_wxyz == NULL: the points as they are).  Bit-identical to the host function (additions in the reference's
 * order -- the sequential float sums are replayed in parallel, exactly; atan2f is glibc 2.35's float algorithm; equal
 * angles of one slice come out in the order libstdc++'s std::sort leaves them in).  histogram_size <= 255.  Slices of
 * any size: up to 4096 points of one 0.2 m slice are processed in LDS, larger ones (the floor of every real scan: 15 000
 * returns of a filtered 64-beam scan) in HBM.  Whether a cloud has such slices is only known on the device; the context
 * enqueues their kernels when the previous cloud had any, and runs a cloud again that needed them without having them.
 * DLIOM_ERR_CAPACITY: |z| >= 409.6 m, non-finite coordinates, more than 63 slices above 4096 points, or std::sort's
 * heap-sort fallback on a segment of more than 8192 elements of such a slice -- use the host function. */
int dliom_cloud_rotational_histogram(dliom_ctx* ctx, const dliom_cloud* cloud, const float rotation_wxyz[4],
                                     int histogram_size, float* histogram);
/* The same in two halves: _begin enqueues the kernels on an auxiliary stream of the context, behind everything the
 * context has been given so far, and returns; the caller may then put other work on the context (the adapter inserts
 * the scan into the submaps, local_trajectory_builder_3d.cc:590-604 -- neither step writes the filtered cloud);
 * _finish waits for the histogram only.  One histogram may be pending per context; the cloud must stay alive until
 * _finish.  Status of the limits (DLIOM_ERR_CAPACITY, see above) comes from _finish. */
int dliom_cloud_rotational_histogram_begin(dliom_ctx* ctx, const dliom_cloud* cloud, const float rotation_wxyz[4],
                                           int histogram_size);
int dliom_cloud_rotational_histogram_finish(dliom_ctx* ctx, float* histogram);
/* Diagnostic: indices of n float keys in the order the device's SortSlice leaves them -- libstdc++'s std::sort
 * on (key, index) pairs compared by key only, EQUAL keys included (introsort's partitions restated as data-parallel
 * rounds, its heap sort at the depth limit, and a stable sort for the final insertion sort).  n <= 4096: the LDS path of
 * the small slices; above: the path of the floor slices (radix sort + the partitions of the segments that hold ties --
 * in LDS on 32-bit (rank, position) items up to ~16 000 keys, on arrays in HBM beyond). */
int dliom_diag_std_sort_order(dliom_ctx* ctx, const float* keys, int n, int32_t* order);
/* Diagnostic: the exact parallel replay of sequential float sums the histogram uses for ComputeCentroid and
 * histogram(bucket) += value (rotational_scan_matcher.cc:49,52-59): k arrays of n floats (values: k x n, row major),
 * sums[i] = (((acc0[i] + v[0]) + v[1]) + ...) in exactly that order, computed by one workgroup per array. */
int dliom_diag_sequential_sums(dliom_ctx* ctx, const float* values, int k, int n, const float* acc0, float* sums);
/* Diagnostic: every `histogram(bucket) += value` of dliom_cloud_rotational_histogram as (bucket, value) in the order of
 * the additions (AddValueToHistogram, rotational_scan_matcher.cc:35-50: slices in key order, points in SortSlice's
 * order).  Stronger than comparing histograms: a bucket whose sum is in the hundreds hides a contribution of 1e-5 that
 * went elsewhere.  Blocking; stores the first `capacity` pairs, *count = how many there are. */
int dliom_diag_histogram_contributions(dliom_ctx* ctx, const dliom_cloud* cloud, const float rotation_wxyz[4],
                                       int histogram_size, int32_t* buckets, float* values, int64_t capacity, int64_t* count);
/* The same with an explicit number of host threads (0 = as many as pay, at most 8; the bits do not depend on it). */
int dliom_rotational_histogram_mt(const float* points_xyz, int64_t n, int histogram_size, int num_threads, float* histogram);
/* RotationalScanMatcher(histograms_at_angles).Match(histogram, initial_angle, angles)
 * (rotational_scan_matcher.cc:174-194), host: one score per angle.  The loop-closure matcher calls
 * the same code to pick the yaw candidates worth discretising. */
int dliom_rotational_scan_match(const float* node_histograms, const float* node_angles, int num_nodes,
                                int histogram_size, const float* scan_histogram, float initial_angle,
                                const float* angles, int num_angles, float* scores);

/* ---- IMU preintegration between scans (host; SURVEY 8f rank 4, PARITY UNPINNED) ------------------
 * Mid-point preintegration with bias Jacobians and covariance as the reference's in-tree
 * IntegrationBase (mapping/internal/3d/initialization/integration_base.h:106-278), plus the VINS-Mono
 * residual it keeps commented out (:280-316) and the matching state prediction -- a self-contained
 * stand-in for the gtsam::PreintegratedImuMeasurements calls of the steady-state path
 * (local_trajectory_builder_3d.cc:179-199).  Blocks of jacobian / covariance (row-major 15 x 15):
 * P 0, R 3, V 6, BA 9, BG 12.  States are [P(3), Q(w,x,y,z), V(3), Ba(3), Bg(3)]; gravity is the
 * world-frame vector G of the residual (e.g. {0, 0, 9.80511}). */
typedef struct dliom_imu_integrator dliom_imu_integrator;
typedef struct dliom_imu_noise { double acc_n, gyr_n, acc_w, gyr_w; } dliom_imu_noise;
typedef struct dliom_imu_preintegration {
  double sum_dt;
  double delta_p[3];
  double delta_q[4];
  double delta_v[3];
  double linearized_ba[3];
  double linearized_bg[3];
  double jacobian[225];
  double covariance[225];
} dliom_imu_preintegration;
int dliom_imu_integrator_create(const double ba[3], const double bg[3], const dliom_imu_noise* noise,
                                dliom_imu_integrator** out);
int dliom_imu_integrator_destroy(dliom_imu_integrator* integrator);
int dliom_imu_integrator_reset(dliom_imu_integrator* integrator, const double ba[3], const double bg[3],
                               const dliom_imu_noise* noise);
int dliom_imu_integrator_push_back(dliom_imu_integrator* integrator, double dt, const double acc[3],
                                   const double gyr[3]);
int dliom_imu_integrator_repropagate(dliom_imu_integrator* integrator, const double ba[3], const double bg[3]);
int dliom_imu_integrator_get(const dliom_imu_integrator* integrator, dliom_imu_preintegration* out);
int dliom_imu_integrator_evaluate(const dliom_imu_integrator* integrator, const double state_i[16],
                                  const double state_j[16], const double gravity[3], double residuals[15]);
int dliom_imu_integrator_predict(const dliom_imu_integrator* integrator, const double state_i[16],
                                 const double gravity[3], double state_j[16]);

/* ---- IMU-LiDAR initialisation (host) ----------------------------------------------------------------
 * The state the steady-state path starts from.  Double arithmetic, every operation rounded on its own, in the order
 * written, parentheses first and otherwise left to right; u . v = (u0*v0 + u1*v1) + u2*v2; u x v = (u1*v2 - u2*v1,
 * u2*v0 - u0*v2, u0*v1 - u1*v0); n(v) = v / sqrt(v . v), component by component.
 *
 * FROM TWO VECTORS (Eigen's Quaternion::FromTwoVectors, general branch, operation for operation): v0 = n(a), v1 = n(b),
 * c = v1 . v0.  For c >= -1 + 1e-12: axis = v0 x v1, s = sqrt((1 + c) * 2), invs = 1 / s, q = (w = s * 0.5, axis * invs).
 * NEARLY OPPOSITE (c < -1 + 1e-12), PARITY UNPINNED AGAINST EIGEN, which takes an SVD there: q = (0, n(v0 x e_k)), half
 * a turn, e_k the coordinate axis on which |v0| is least (ties: the lowest k).
 * The rotation matrix of q is Eigen's toRotationMatrix: tx = 2*x, ty = 2*y, tz = 2*z, twx = tx*w, twy = ty*w, twz = tz*w,
 * txx = tx*x, txy = ty*x, txz = tz*x, tyy = ty*y, tyz = tz*y, tzz = tz*z; rows (1 - (tyy + tzz), txy - twz, txz + twy),
 * (txy + twz, 1 - (txx + tzz), tyz - twx), (txz - twy, tyz + twx, 1 - (txx + tyy)).
 *
 * dliom_imu_static_initialization: LocalTrajectoryBuilder3D::InitializeStatic (local_trajectory_builder_3d.cc:203-229) for
 * a platform at rest.  acc and gyr hold n samples (x, y, z each).  The sums run from +0.0 in sample order; acc_mean and
 * gyro_mean are the sums / (double)n.  g_vec = (0, 0, -gravity_norm).  R = the matrix of FROM TWO VECTORS (acc_mean,
 * -g_vec): IMU frame to world, row-major in rotation9.  ba = R^T g_vec + acc_mean, a component
 * ((R0a*g0 + R1a*g1) + R2a*g2) + acc_mean_a; bg = gyro_mean; position = velocity = 0.
 * DLIOM_ERR_INVALID_ARGUMENT: NULLs, n <= 0, a non-finite sample, a non-finite or non-positive gravity_norm, an
 * acc_mean without a direction. */
int dliom_imu_static_initialization(int64_t n, const double* acc, const double* gyr, double gravity_norm, double rotation9[9],
                                    double ba[3], double bg[3], double position[3], double velocity[3]);
/* dliom_imu_lidar_initialization: Initializer::Initialization (initialization/imu_lidar_initializer.cc:50-229) on N frames
 * (F + 1 of them in the caller's terms).  A frame is a pose T_li of the laser in the first laser frame
 * [tx, ty, tz, qw, qx, qy, qz] and the preintegration that was running when it was stored (sum_dt, delta_p, delta_v of
 * dliom_imu_integrator_get); frame 0 may carry none, and its own is never read.  R_i is the rotation matrix of the frame's
 * quaternion as it stands (FROM TWO VECTORS above), T_i its translation, tlb the translation of transform_lb, whose
 * rotation the reference reads and does not use.  A pair is (i, j = i + 1) with a preintegration on j; pairs without are
 * skipped.  dt = sum_dt of j.  THE SOLVER is the library's own (Gaussian elimination with partial pivoting by rows, back
 * substitution left to right), PARITY UNPINNED AGAINST EIGEN's pivoted LDLT; it is pinned against numpy.linalg.solve within
 * 64 * cond(A) * 2^-52 * |x| a solve (tests/test_imu_lidar_init_host.py).
 *   ApproximateGravity (:50-124).  N < 7: DLIOM_INIT_TOO_FEW_FRAMES.  Unknowns: the frames' velocities in their own frames
 *   (3 N), then g (3).  A pair's 6 x 9 block M over (V_i, V_j, g) and its right-hand side r:
 *     rows 0-2: (-dt I | 0 | R_i^T * (dt*dt/2)),   r = ((delta_p + (R_i^T R_j) tlb) - tlb) - R_i^T (T_j - T_i)
 *     rows 3-5: (-I | R_i^T R_j | R_i^T * dt),     r = delta_v
 *   M^T M and M^T r (sums over the six rows in row order) are added at the columns of V_i, V_j and g.  Then A and b are
 *   multiplied by 1000 and solved; g = the last three unknowns.  | |g| - gravity_norm | < 1.0, else DLIOM_INIT_GRAVITY_NORM.
 *   TangentBasis (:36-48): a = n(g0); tmp = (0, 0, 1), or (1, 0, 0) if a == (0, 0, 1) exactly; b = n(tmp - a * (a . tmp)),
 *   c = a x b.
 *   RefineGravity (:126-211).  g0 = n(g) * gravity_norm.  Unknowns: the velocities (3 N), then (d0, d1).  A and b are zeroed
 *   ONCE, before four passes, and NOT between them: every pass adds its blocks to the already scaled system of the pass
 *   before.  That is what the reference's binary does.  A pass: (lx, ly) = TangentBasis(g0); a pair's 6 x 8 block with
 *   L = [lx ly]:
 *     rows 0-2: (-dt I | 0 | (R_i^T L) * (dt*dt/2)),  r = (((delta_p + (R_i^T R_j) tlb) - tlb) - (R_i^T g0) * (dt*dt/2)) - R_i^T (T_j - T_i)
 *     rows 3-5: (-I | R_i^T R_j | (R_i^T L) * dt),    r = delta_v - (R_i^T g0) * dt
 *   added as above; A and b times 1000; solved; g0 = n(g0 + (lx * d0 + ly * d1)) * gravity_norm.
 *   After the four passes gravity = g0 and velocities = the last solve's first 3 N unknowns (each in its own frame);
 *   | |g| - gravity_norm | < 0.2, else DLIOM_INIT_GRAVITY_NORM.  A system without a pivot: DLIOM_INIT_SINGULAR.
 * *outcome is a DLIOM_INIT_* value; the call returns DLIOM_OK whenever its arguments were well formed.
 *
 * dliom_imu_lidar_align_with_world: LocalTrajectoryBuilder3D::AlignWithWorld (local_trajectory_builder_3d.cc:1010-1086), in
 * its order, F = num_frames - 1:
 *   1. Excitation.  Over the F later frames (those without a preintegration skipped): t = delta_v / sum_dt; sum from ZERO
 *      (the reference leaves sum_g uninitialised); mean = sum * 1.0 / F; var = the sum of (t - mean) . (t - mean);
 *      *excitation = sqrt(var / F).  Below 0.25: DLIOM_INIT_NO_EXCITATION.
 *   2. The call above; its outcome if it is not DLIOM_INIT_OK.  gravity_in_laser is its g.
 *   3. Per frame: T_li * transform_lb: P_i = R_li t_lb + T_i; R_i = the matrix of (q_li q_lb) / |q_li q_lb| (Hamilton
 *      product, each component's four terms left to right); V_i = R_i V_i.
 *   4. g_base = -g; world_rotation9 = the matrix of FROM TWO VECTORS (n(g_base), (0, 0, -1)); P_i, R_i and V_i are turned by
 *      it from the left.
 * positions and velocities hold 3, rotations 9 doubles a frame (row-major); they are written only under DLIOM_INIT_OK.
 * DLIOM_ERR_INVALID_ARGUMENT for both calls: NULLs, fewer than 1 (align: 2) or more than DLIOM_INIT_MAX_FRAMES frames,
 * non-finite input, a preintegration with sum_dt <= 0, a non-positive gravity_norm. */
#define DLIOM_INIT_MAX_FRAMES 64
enum {
  DLIOM_INIT_OK = 0,
  DLIOM_INIT_NO_EXCITATION = 1,
  DLIOM_INIT_TOO_FEW_FRAMES = 2,
  DLIOM_INIT_GRAVITY_NORM = 3,
  DLIOM_INIT_SINGULAR = 4
};
typedef struct dliom_init_frame {
  double pose[7];
  int has_preintegration;
  int reserved;              /* 0 */
  double sum_dt, delta_p[3], delta_v[3];
} dliom_init_frame;
int dliom_imu_lidar_initialization(const dliom_init_frame* frames, int num_frames, const double transform_lb[7],
                                   double gravity_norm, double* velocities, double gravity[3], int* outcome);
int dliom_imu_lidar_align_with_world(const dliom_init_frame* frames, int num_frames, const double transform_lb[7],
                                     double gravity_norm, double* positions, double* rotations, double* velocities,
                                     double gravity_in_laser[3], double world_rotation9[9], double* excitation, int* outcome);

/* ---- LocalTrajectoryBuilder3D::WindowOptimize: IMU-preintegration cost in the optimisation ----------
 * (host; PARITY UNPINNED: GTSAM 4.0.2 is not in the reference tree and the reference has no
 * test at this boundary).  Replaces mapping/internal/3d/local_trajectory_builder_3d.cc:693-863 and the
 * gtsam::PreintegratedImuMeasurements calls of AddImuData (:179-199): IMU preintegration (tangent form like the
 * reference's GTSAM build, or the manifold form: options.tangent_preintegration), ImuFactor +
 * bias BetweenFactor + PriorFactor<Pose3> on the matched pose + Pose3GravityFactor
 * (gravity_factor/gravity_factor.cc:10-33), solved as a fixed-lag Gauss-Newton smoother with marginalisation
 * in place of ISAM2.  Poses are [x, y, z, qw, qx, qy, qz], biases [ax, ay, az, gx, gy, gz].
 * Call order per scan, as the reference's AddImuData / AddRangeData / WindowOptimize:
 *   _add_imu (every IMU sample) ... _predict (initial pose for the matchers) ... _add_pose (matched pose)
 * DLIOM_ERR_DIVERGED mirrors FailureDetection (:856-859,896-913): |v| > 30 m/s or a bias norm > 1 after a scan.  The
 * outputs hold that scan's estimate and, like ResetParams(), the window only forgets that its graph was started: the next
 * _window_optimize starts a new graph at that estimate with the initial priors (the reference does exactly this and goes
 * on); a caller may re-initialise instead. */
#define DLIOM_ERR_DIVERGED (-11)
/* add_pose returns DLIOM_ERR_SOLVER when the normal equations cannot be factorised: the window is then exactly as before
 * the call (the new key, its factors and the gravity estimator's entry are taken back, the running preintegration kept). */
typedef struct dliom_imu_window dliom_imu_window;
typedef struct dliom_imu_window_options {
  double acc_noise, gyr_noise, acc_bias_noise, gyr_bias_noise; /* trajectory_builder_3d.lua:88-91 */
  double gravity;                                               /* :92, n_gravity = (0, 0, -gravity) */
  double integration_sigma;                                     /* 1e-4, local_trajectory_builder_3d.cc:81-82 */
  double prior_pose_noise;                                      /* lua :93 */
  double prior_velocity_sigma, prior_bias_sigma;                /* 1e4 / 1e-2, .cc:88-89 */
  double ceres_pose_noise_t, ceres_pose_noise_r;                /* lua :96-97 */
  double ceres_pose_noise_t_drift, ceres_pose_noise_r_drift;    /* lua :98-99 (is_drift) */
  double prior_gravity_noise;                                   /* lua :100 */
  int window_size;  /* 0: the reference's rule -- EVERY key since the last graph reset stays in the problem (needs
                       graph_reset_every >= 2), linearisation points move by relinearize_threshold, nothing is
                       marginalised (.cc:693-863 with ISAM2 as it is parameterised at :676-679);
                       2..4096: fixed-lag Gauss-Newton smoother, older states marginalised (Schur complement) */
  int iterations;   /* Gauss-Newton iterations per scan (the reference calls ISAM2::update twice) */
  int enable_gravity_factor;               /* lua :31 (false; dlio/config/basic_config_3d.lua:80 true): EstimateGravity per
                                              scan and, when it succeeds, a Pose3GravityFactor (.cc:819-831) */
  int frames_for_online_gravity_estimate;  /* lua :29 (7): estimator window, and the factor's key distance; needs
                                              window_size >= this + 1 */
  double lidar_in_imu_translation[3];      /* transform_lb_.translation() (.cc:1140), zero if the poses are the IMU's */
  int graph_reset_every;                   /* submaps.num_range_data (.cc:749-792): when key_ reaches it the reference
                                              replaces its graph by the newest state with the marginal covariances of
                                              pose, velocity and bias taken separately; 0 = never (plain fixed-lag
                                              smoothing, which keeps the cross-covariances that reset drops); >= 2 */
  int tangent_preintegration;              /* 1 (default): gtsam::TangentPreintegration, what PreintegratedImuMeasurements
                                              IS in the reference's build (README.MD:13-15 builds GTSAM 4.0.2 without
                                              -DGTSAM_TANGENT_PREINTEGRATION=OFF; 4.0.x defaults to ON): [theta, p, v]
                                              integrated in the tangent space of the first state, error = local
                                              coordinates of the predicted state at state j.  0: the manifold form of
                                              Forster et al. (GTSAM with the flag OFF).  Still PARITY UNPINNED either way */
  double relinearize_threshold;            /* window_size == 0 only: ISAM2Params::relinearizeThreshold (.cc:677, 0.1): a key's
                                              linearisation point -- X(i), V(i) and B(i) each by itself -- moves to its estimate
                                              when a component of ITS increment exceeds it (checked at each of the `iterations`
                                              updates, relinearizeSkip = 1); the
                                              estimate is linearisation point (+) increment, the increments solving the
                                              linearised problem exactly.  0 = every update relinearises every key = batch
                                              Gauss-Newton over the whole graph (oracle/imu_window_ref.py's
                                              ReferenceRuleSmoother idealisation) */
} dliom_imu_window_options;
int dliom_imu_window_default_options(dliom_imu_window_options* options);
int dliom_imu_window_create(const dliom_imu_window_options* options, dliom_imu_window** out);
int dliom_imu_window_destroy(dliom_imu_window* window);
/* InitializeIMU (:331-356) + the priors of the gtsam_initialized_ == false branch (:712-745): prev_state_ / prev_bias_,
 * X(0), V(0), B(0) with their priors */
int dliom_imu_window_initialize(dliom_imu_window* window, const double pose7[7], const double velocity[3],
                                const double bias6[6]);
/* imu_integrator_opt_->integrateMeasurement(acc, gyr, dt) (:188-196) */
int dliom_imu_window_add_imu(dliom_imu_window* window, const double acc[3], const double gyr[3], double dt);
/* the same for n samples (acc, gyr: n x 3; dt: n) in one call: for callers that buffer the IMU between two scans */
int dliom_imu_window_add_imu_batch(dliom_imu_window* window, int n, const double* acc, const double* gyr, const double* dt);
/* imu_integrator_opt_->predict(prev_state_, prev_bias_) (:198-199) */
int dliom_imu_window_predict(const dliom_imu_window* window, double pose7[7], double velocity[3]);
/* Pose3GravityFactor on the state `states_back` keys before the newest (:819-831); direction = estimated gravity */
int dliom_imu_window_add_gravity(dliom_imu_window* window, int states_back, const double direction[3]);
/* WindowOptimize(matched_pose, is_drift): new key, factors, optimisation; outputs prev_pose_ / prev_vel_ / prev_bias_ */
int dliom_imu_window_add_pose(dliom_imu_window* window, const double matched_pose7[7], int is_drift, double pose7[7],
                              double velocity[3], double bias6[6]);
/* Work done by the solver so far: linearisation points moved, chain blocks (states) eliminated -- what a scan costs */
int dliom_imu_window_solver_stats(const dliom_imu_window* window, int64_t* relinearizations, int64_t* blocks_eliminated);
/* WindowOptimize as the reference calls it, once per scan, the first call after _initialize included: that call only
 * starts the graph (gtsam_initialized_ == false, .cc:712-745: priors at the initial state, the preintegration since
 * InitializeIMU dropped) and returns the initial state -- the scan's matched pose is not used, as in the reference; every
 * later call is dliom_imu_window_add_pose.  (_add_pose alone adds a key on every call: the primitive the solver tests use.) */
int dliom_imu_window_window_optimize(dliom_imu_window* window, const double matched_pose7[7], int is_drift, double pose7[7],
                                     double velocity[3], double bias6[6]);
int dliom_imu_window_state(const dliom_imu_window* window, int states_back, double pose7[7], double velocity[3],
                           double bias6[6]);
int dliom_imu_window_size(const dliom_imu_window* window);
/* Diagnostic: Jacobian (15 x 30, row major) of the IMU factor + bias random walk between the window's two newest
 * states -- the closed form the solver uses and central differences of its residual.  Needs >= 2 states. */
int dliom_diag_imu_factor_jacobians(dliom_imu_window* window, double* analytic, double* numeric);
/* g_vec_est_G_ of the last EstimateGravity() (local_trajectory_builder_3d.cc:1106-1154), whether that call passed the
 * reference's gates, and how many gravity factors add_pose has added so far */
int dliom_imu_window_gravity_estimate(const dliom_imu_window* window, double gravity_in_global[3], int* valid,
                                      int64_t* factors_added);
/* GravityEstimator::Estimate (gravity_factor/gravity_estimator.cc:172-188) on explicit frames: pose [t, q(wxyz)] relative to
 * the first frame, the preintegration stored WITH each frame (deltaTij, deltaPij, deltaVij) and its body-frame velocity.
 * gravity_out is in the first frame (the reference's sign: it points up); *accepted = the function's return value. */
int dliom_gravity_estimate(int num_frames, const double* poses7, const double* delta_t, const double* delta_p,
                           const double* delta_v, const double* velocities, const double lidar_in_imu_translation[3],
                           double gravity_norm, double gravity_out[3], int* accepted);

/* ---- RealTimeCorrelativeScanMatcher2D (BASELINE config 1: host only, by contract) -------------
 * double Match(initial_pose_estimate, point_cloud, probability_grid, pose_estimate)
 * (mapping/internal/2d/scan_matching/real_time_correlative_scan_matcher_2d.h:66-69, .cc:74-108).
 * Poses are [x, y, theta].  The ProbabilityGrid is passed as what it stores: num_x_cells *
 * num_y_cells uint16 correspondence-cost cells, row-major num_x_cells * y + x
 * (mapping/2d/grid_2d.cc:168-171), with MapLimits{resolution, max} (mapping/2d/map_limits.h). */
int dliom_rtcsm2d_match(const dliom_rtcsm_options* options, const double initial_pose_estimate[3],
                        const float* points_xyz, int64_t n, const uint16_t* correspondence_cost_cells,
                        int num_x_cells, int num_y_cells, double resolution, double max_x, double max_y,
                        double pose_estimate[3], double* score);

/* ---- diagnostics used by the parity tests and bench.py ------------------------
 * These expose intermediate results of the same device code the matchers run. */
/* Cell index of R(pose)*p + t per point, computed by the score kernel's own
 * device function (bit-exactness probe for hybrid_grid.h:430-435). */
int dliom_probe_transform_cell_indices(dliom_ctx* ctx, const float pose[7],
                                       const float* points_xyz, int64_t n, float resolution,
                                       int32_t* cell_xyz);
/* Per candidate (generation order) the exact integer sum over points of
 * max(value & 0x7fff, 1): the order-independent score volume. */
int dliom_rtcsm3d_score_volume(dliom_ctx* ctx, const dliom_rtcsm_options* options,
                               const double initial_pose_estimate[7], const float* points_xyz,
                               int64_t n, const dliom_grid* grid, uint64_t* sums,
                               int64_t capacity, int64_t* num_candidates);
/* For k given candidates: the reference's SEQUENTIAL float sum of probabilities in point order
 * (rtcsm_3d.cc:101-104, before the division by N), method 0 = one lane replays the loop,
 * method 1 = the binade-wise exact parallel scan over elements, method 2 = the same scan over
 * precomputed 64-point chunk functions (both n <= 65536).  All three must be bit-identical. */
int dliom_rtcsm3d_sequential_sums(dliom_ctx* ctx, const dliom_rtcsm_options* options,
                                  const double initial_pose_estimate[7], const float* points_xyz, int64_t n,
                                  const dliom_grid* grid, const int64_t* candidate_indices, int64_t k,
                                  int method, float* sums);
/* One evaluation of the stacked problem at `pose`: cost = 1/2 sum r^2,
 * gradient[6] = J^T r and jtj[36] = J^T J (row-major) in the 6-dof tangent
 * space of (translation, QuaternionParameterization). */
int dliom_csm3d_evaluate(dliom_ctx* ctx, const dliom_csm_options* options,
                         const double target_translation[3],
                         const double initial_pose_estimate[7], const double pose[7],
                         int num_clouds, const float* const* points_xyz, const int64_t* n,
                         const dliom_grid* const* grids, double* cost, double gradient[6],
                         double jtj[36]);

/* ---- pose graph optimisation ------------------------------------------------------------------
 * OptimizationProblem3D::Solve (mapping/internal/optimization/optimization_problem_3d.cc:259-589) as this fork runs
 * it: the IMU, odometry and local-SLAM terms are commented out there (:350-489) and the inter-submap loss is
 * TrivialLoss (:336-338), so the problem is one SpaCostFunction3D a constraint (cost_functions/spa_cost_function_3d.h:
 * 46-56, cost_helpers_impl.h:57-101, transform/transform.h:59-81) between ONE submap pose and ONE node pose.  The
 * *_terms entry points below add the fixed-frame pose constraints (:491-548, live code in the fork) and upstream's
 * HuberLoss on the inter-submap constraints, the *_landmarks entry points further the landmark observations
 * (AddLandmarkCostFunctions, :124-186).  The 2D problem is not covered.
 *
 * Poses are [tx ty tz qw qx qy qz].  Parameter blocks (:279-330, ceres_pose.cc): a translation block with no
 * parameterisation, or SubsetParameterization(3, {2}) under fix_z_in_3d; a rotation block with
 * QuaternionParameterization.  `gravity_aligned_submap` (the first submap in MapById order, or -1 for none) keeps its
 * translation constant and moves its rotation by ConstantYawQuaternionPlus (mapping/internal/3d/
 * rotation_parameterization.h:41-62).  submap_constant[i] / node_constant[i] != 0: both blocks constant (a frozen
 * trajectory, :310-315,325-329).  A NULL constant array means none.
 *
 * The solver is ceres::Solve as common/ceres_solver_options.cc:35-42 configures it (Ceres 1.13 defaults otherwise):
 * trust region, Levenberg-Marquardt, Jacobi scaling, tolerances 1e-6 / 1e-10 / 1e-8.  As in Ceres (its behaviour, not
 * the tree's) constant blocks, blocks no constraint touches and constraints whose four blocks are all constant leave
 * the reduced problem; the cost of the latter is added to the summary's costs as a fixed cost.
 *
 * The nodes are eliminated (their Hessian is block-diagonal) and the dense reduced system over the submaps is
 * factorised on the device in FP64.  Its dimension (summary->reduced_dimension: the free tangent columns of the
 * submaps) is capped at DLIOM_POSE_GRAPH_MAX_REDUCED_DIMENSION = 8192 (about 1 365 free submaps, 512 MB): beyond it,
 * or with index arrays beyond 2^31 - 1 entries, DLIOM_ERR_TOO_LARGE.  Scratch is allocated and released inside the
 * call: dliom_ctx_memory_stats is unchanged by it.  DLIOM_ERR_INVALID_ARGUMENT: NULL pointers, negative counts, a
 * constraint index or gravity_aligned_submap out of range.  DLIOM_ERR_SOLVER: where Ceres would report FAILURE (a
 * non-finite input pose or constraint, five invalid steps in a row); the poses are then left as they were.  A
 * non-finite candidate cost is a rejected step, not an error.  Refusals of the arguments (the three statuses above,
 * a non-finite input) happen before anything is launched.
 * Every sum is taken in a fixed order without floating-point atomics: two solves of one input give the same bits. */
#define DLIOM_ERR_TOO_LARGE (-14)
#define DLIOM_POSE_GRAPH_MAX_REDUCED_DIMENSION 8192
#define DLIOM_POSE_GRAPH_MAX_RECORDED_STEPS 256
typedef struct dliom_pose_graph_options {
  int fix_z_in_3d;            /* optimization_problem_options.proto fix_z_in_3d */
  int use_nonmonotonic_steps; /* common.proto.CeresSolverOptions */
  int max_num_iterations;     /* ... (SetMaxNumIterations, pose_graph_3d.cc:677-682) */
  int num_threads;            /* accepted, unused */
} dliom_pose_graph_options;
/* OptimizationProblem3D::Constraint (pose_graph_interface.h): zbar = the node's pose in the submap frame. */
typedef struct dliom_pose_graph_constraint {
  int32_t submap;
  int32_t node;
  double zbar[7];
  double translation_weight;
  double rotation_weight;
} dliom_pose_graph_constraint;
typedef struct dliom_pose_graph_summary {
  double initial_cost;
  double final_cost;
  int num_successful_steps;
  int num_unsuccessful_steps;
  int num_iterations;
  int num_residual_evaluations;
  int num_jacobian_evaluations;
  int termination_type; /* 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE */
  int reduced_dimension;
  int linear_solver_failures; /* factorisations that met a non-positive pivot (each an invalid step) */
  /* milliseconds a stage took, summed over the iterations; filled (and the stages separated by stream
   * synchronisations) only while the context's profiling is on */
  double linearise_ms, eliminate_ms, factor_ms, back_substitute_ms, host_ms;
  /* iterations 1 .. num_recorded_steps: 1 successful, 0 unsuccessful, 2 invalid */
  int num_recorded_steps;
  unsigned char steps[DLIOM_POSE_GRAPH_MAX_RECORDED_STEPS];
} dliom_pose_graph_summary;
/* void OptimizationProblem3D::Solve(constraints, frozen_trajectories, landmark_nodes) (optimization_problem_3d.cc:
 * 259-589) on compacted indices: submap_poses7 / node_poses7 are read and, on DLIOM_OK, overwritten with the best
 * iterate (blocks outside the reduced problem keep their bits). */
int dliom_pose_graph_solve(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps, double* submap_poses7,
                           const unsigned char* submap_constant, int gravity_aligned_submap, int num_nodes,
                           double* node_poses7, const unsigned char* node_constant, int64_t num_constraints,
                           const dliom_pose_graph_constraint* constraints, dliom_pose_graph_summary* summary);
/* Diagnostics in the style of dliom_csm3d_evaluate.  One evaluation at the given poses: *cost = 1/2 sum r^2 of the
 * reduced problem plus the fixed cost, residuals[6 * c ..] of every constraint (cost_helpers_impl.h:57-101), and the
 * gradient J^T r in the tangent space: 6 slots a pose, submaps first, [translation | rotation]; a slot outside the
 * reduced problem (constant, fix_z's z, the gravity-aligned submap's third) holds 0.  Any output may be NULL. */
int dliom_pose_graph_evaluate(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                              const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                              int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                              int64_t num_constraints, const dliom_pose_graph_constraint* constraints, double* cost,
                              double* residuals, double* gradient);
/* The trust-region step of iteration 1 (levenberg_marquardt_strategy.cc with the iteration-0 Jacobi scaling) for the
 * given radius: delta[6 * (num_submaps + num_nodes)] in the slots of `gradient` above, already multiplied by the column
 * scaling (what Plus receives), and *model_cost_change.  DLIOM_ERR_SOLVER when the factorisation fails. */
int dliom_pose_graph_step(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                          const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                          int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                          int64_t num_constraints, const dliom_pose_graph_constraint* constraints, double radius,
                          double* delta, double* model_cost_change, int* reduced_dimension);

/* Further terms of OptimizationProblem3D::Solve.  A NULL pointer to this struct, and a struct of 0 fixed frames and
 * huber_scale 0, are the entry points above, bit for bit (those are calls of the ones below with NULL).
 *
 * Fixed frames (optimization_problem_3d.cc:491-548): one block a trajectory with fixed-frame pose data (GPS).  Its
 * translation has NO parameterisation -- three columns even under fix_z_in_3d -- and its rotation moves by
 * AutoDiffLocalParameterization<YawOnlyQuaternionPlus, 4, 1> (rotation_parameterization.h:27-39): one column, tangent
 * slot 3, Plus = [sqrt(1 - d^2), 0, 0, d] (x) q with d = clamp(delta, -0.5, 0.5).  That is applied to whatever rotation
 * is given; starting the block yaw-only is the caller's business (:529-533).  A fixed frame is never constant, also
 * on a frozen trajectory (the fork does not skip those in this loop).  A fixed-frame constraint is a
 * dliom_pose_graph_constraint whose .submap is the fixed frame's index: the same SpaCostFunction3D with the fixed frame
 * in the submap's place, never under a loss (:541-546).  The fixed frames' columns follow the submaps' in the reduced
 * system, four a frame, and count against DLIOM_POSE_GRAPH_MAX_REDUCED_DIMENSION.  Residual blocks are ordered
 * constraints first, then fixed-frame constraints.
 *
 * Loss: huber_scale == 0 is the fork's TrivialLoss; > 0 puts ceres::HuberLoss(huber_scale) (upstream :335-338,
 * optimization_problem_options.proto huber_scale) on the constraints c with inter_submap[c] != 0 (Constraint::tag ==
 * INTER_SUBMAP; NULL: none).  Ceres 1.13 restated: s = ||r||^2 of the block, b = huber_scale^2; for s > b the block's
 * cost is 1/2 (2 a sqrt(s) - b) and residual and Jacobian are scaled by sqrt(rho') with rho' = max(DBL_MIN, a / sqrt(s))
 * (Corrector with rho'' <= 0).  Costs, residuals and gradients reported below are the corrected ones, as
 * Problem::Evaluate reports them.
 *
 * Beyond the refusals above: DLIOM_ERR_INVALID_ARGUMENT for a negative count, a positive count with a NULL array, a
 * fixed-frame or node index out of range, a negative or non-finite huber_scale; DLIOM_ERR_SOLVER for a non-finite
 * fixed-frame pose or constraint; all before anything is launched. */
typedef struct dliom_pose_graph_terms {
  int num_fixed_frames;
  double* fixed_frame_poses7; /* the start value; solve overwrites it with the best iterate on DLIOM_OK */
  int64_t num_fixed_frame_constraints;
  const dliom_pose_graph_constraint* fixed_frame_constraints;
  double huber_scale;
  const unsigned char* inter_submap; /* num_constraints flags, or NULL */
} dliom_pose_graph_terms;
int dliom_pose_graph_solve_terms(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps, double* submap_poses7,
                                 const unsigned char* submap_constant, int gravity_aligned_submap, int num_nodes,
                                 double* node_poses7, const unsigned char* node_constant, int64_t num_constraints,
                                 const dliom_pose_graph_constraint* constraints, const dliom_pose_graph_terms* terms,
                                 dliom_pose_graph_summary* summary);
/* residuals: 6 a residual block, the constraints and then the fixed-frame constraints; gradient: 6 slots a pose, the
 * submaps, the nodes and then the fixed frames (slots 0..2 the translation, slot 3 the yaw, 4 and 5 hold 0). */
int dliom_pose_graph_evaluate_terms(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                                    const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                                    int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                                    int64_t num_constraints, const dliom_pose_graph_constraint* constraints,
                                    const dliom_pose_graph_terms* terms, double* cost, double* residuals, double* gradient);
/* delta: in the slots of `gradient` above. */
int dliom_pose_graph_step_terms(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                                const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                                int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                                int64_t num_constraints, const dliom_pose_graph_constraint* constraints,
                                const dliom_pose_graph_terms* terms, double radius, double* delta, double* model_cost_change,
                                int* reduced_dimension);

/* Landmark observations (optimization_problem_3d.cc:124-186, cost_functions/landmark_cost_function_3d.h).  A NULL pointer
 * to dliom_pose_graph_landmarks, and a struct of 0 landmarks and 0 observations, are the *_terms entry points, bit for
 * bit (those are calls of the ones below with NULL).
 *
 * Every used observation of a landmark is one residual block without a loss over six parameter blocks -- rotation and
 * translation of the node before the observation (prev), of the node after it (next) and of the landmark:
 *   e = ScaleError(ComputeUnscaledError(landmark_to_tracking, slerp(prev.q, next.q, t), prev.p + t (next.p - prev.p),
 *                                       landmark.q, landmark.p), translation_weight, rotation_weight)
 * (cost_helpers_impl.h:57-153) with t = (observation.time - prev.time) / (next.time - prev.time), which the caller
 * computes (interpolation_parameter).
 *   SlerpQuaternions is restated exactly: cos_theta = p0 n0 + p1 n1 + p2 n2 + p3 n3 in that order; for
 *   |cos_theta| < 1 - 1e-5, theta = acos(|cos_theta|), prev_scale = sin((1 - t) theta) / sin(theta), next_scale =
 *   sin(t theta) / sin(theta); otherwise the linear scales 1 - t and t; next_scale changes sign when cos_theta < 0; the
 *   result prev_scale p + next_scale n is NOT renormalised.
 *   The landmark block is CeresPose(start, nullptr, QuaternionParameterization): its translation has NO
 *   parameterisation -- three columns also under fix_z_in_3d, as for a fixed frame -- and its rotation moves by
 *   QuaternionParameterization.  The nodes keep theirs: a node drops its z column under fix_z_in_3d.
 *   landmark_constant[l] != 0: both blocks of landmark l are constant (NULL: none).  The reference sets this for every
 *   landmark when frozen_trajectories is non-empty (:169-174) and then skips the landmarks that have no
 *   global_landmark_pose (:131-134); both rules, like finding prev and next (:137-154), are the caller's business.
 *   Ceres' removal rules extend unchanged: a constant block, or a block no remaining residual block uses, leaves the
 *   problem; an observation whose six blocks are all constant contributes only to the fixed cost.
 *   Residual block order, which is the input order of every segmented sum: the constraints, the fixed-frame
 *   constraints, then the observations in input order.
 *
 * A landmark residual couples two nodes, so those nodes cannot stay in the block-diagonal elimination: every
 * non-constant node that a remaining observation names is "promoted" into the dense reduced system, six columns (five
 * under fix_z_in_3d), and so is every non-constant landmark, six columns.  The columns are ordered submaps, fixed
 * frames, promoted nodes, landmarks, and all count against DLIOM_POSE_GRAPH_MAX_REDUCED_DIMENSION (so at most about
 * 1 365 promoted nodes and landmarks together with no submap free).  Landmarks are kept, not eliminated.
 *
 * Beyond the refusals above, all before anything is launched: DLIOM_ERR_INVALID_ARGUMENT for a negative count, a
 * positive count with a NULL array, a landmark or node index out of range, prev_node == next_node;
 * DLIOM_ERR_SOLVER for a non-finite interpolation_parameter, landmark pose, weight or transform. */
typedef struct dliom_pose_graph_landmark_observation {
  int32_t landmark, prev_node, next_node; /* prev_node != next_node */
  double interpolation_parameter;         /* t, finite */
  double landmark_to_tracking7[7];
  double translation_weight, rotation_weight;
} dliom_pose_graph_landmark_observation;
typedef struct dliom_pose_graph_landmarks {
  int num_landmarks;
  double* landmark_poses7;                /* start values; solve overwrites them with the best iterate on DLIOM_OK */
  const unsigned char* landmark_constant; /* or NULL */
  int64_t num_observations;
  const dliom_pose_graph_landmark_observation* observations;
} dliom_pose_graph_landmarks;
int dliom_pose_graph_solve_landmarks(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps, double* submap_poses7,
                                     const unsigned char* submap_constant, int gravity_aligned_submap, int num_nodes,
                                     double* node_poses7, const unsigned char* node_constant, int64_t num_constraints,
                                     const dliom_pose_graph_constraint* constraints, const dliom_pose_graph_terms* terms,
                                     const dliom_pose_graph_landmarks* landmarks, dliom_pose_graph_summary* summary);
/* residuals: 6 a residual block -- the constraints, the fixed-frame constraints, then the observations; gradient: 6
 * slots a pose -- the submaps, the nodes, the fixed frames, then the landmarks. */
int dliom_pose_graph_evaluate_landmarks(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                                        const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                                        int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                                        int64_t num_constraints, const dliom_pose_graph_constraint* constraints,
                                        const dliom_pose_graph_terms* terms, const dliom_pose_graph_landmarks* landmarks, double* cost,
                                        double* residuals, double* gradient);
/* delta: in the slots of `gradient` above. */
int dliom_pose_graph_step_landmarks(dliom_ctx* ctx, const dliom_pose_graph_options* options, int num_submaps,
                                    const double* submap_poses7, const unsigned char* submap_constant, int gravity_aligned_submap,
                                    int num_nodes, const double* node_poses7, const unsigned char* node_constant,
                                    int64_t num_constraints, const dliom_pose_graph_constraint* constraints,
                                    const dliom_pose_graph_terms* terms, const dliom_pose_graph_landmarks* landmarks, double radius,
                                    double* delta, double* model_cost_change, int* reduced_dimension);
/* GetInitialLandmarkPose (optimization_problem_3d.cc:106-122) on the host in double: the pose interpolated between prev
 * and next at t, times landmark_to_tracking -- a landmark's start value from its first used observation.  No context. */
int dliom_pose_graph_initial_landmark_pose(const double* prev_pose7, const double* next_pose7, double t,
                                           const double* landmark_to_tracking7, double* out7);

/* ---- submap feature matching -------------------------------------------------------------------
 * The second half of ConstraintBuilder3D::ExtractFeaturesForSubmap (mapping/internal/constraints/
 * constraint_builder_3d.cc:459-529): which earlier submaps a finished submap is matched against (`matched_submaps`),
 * from the key points and descriptors the caller's SURF produced.  PARITY UNPINNED AGAINST OPENCV: the reference's
 * matcher is FLANN (randomised, approximate) and estimateAffinePartial2D draws from OpenCV's RNG, so its result cannot
 * be pinned.  What is pinned, bit for bit against a CPU model (tests/cpp/feature_match_model.cc), is this definition:
 *
 * Nearest neighbours.  Descriptors have D floats, D a multiple of 4, 4 <= D <= 128.  s(i, j) is a float accumulated in
 * dimension order d = 0 .. D-1 from 0.0f: diff = q[d] - t[d]; s = fmaf(diff, diff, s).  The nearest neighbour j0 of
 * query i is the j with the least s, ties to the lowest j; the second nearest j1 is the same rule over j != j0.
 * d0 = sqrtf(s(i, j0)), d1 = sqrtf(s(i, j1)), correctly rounded.  A pair of sets is matched only if both hold >= 2 key
 * points (:476-477), else DLIOM_FEATURE_TOO_FEW_KEYPOINTS.
 *
 * Good matches (:485-491).  Match i is good iff (double)d0 < r * (double)d1, r = good_match_ratio_of_distance; good
 * matches keep query order.  Fewer than minimum_good_match_num: DLIOM_FEATURE_TOO_FEW_GOOD_MATCHES (:493).  More than
 * DLIOM_FEATURE_MAX_GOOD: DLIOM_ERR_CAPACITY as that pair's status.
 *
 * Points (:494-504), floats as in cv::Point2f: from.x = (float)ox_q + (float)((double)kp_q[i].x * resolution_q),
 * to.x = (float)ox_t + (float)((double)kp_t[j0].x * resolution_q), likewise y.  Both sides take the QUERY set's
 * resolution, as the reference does.  Everything below is double arithmetic on these floats, every operation rounded
 * on its own (no contraction), in the order written.
 *
 * Hypotheses, our statement of estimateAffinePartial2D(from, to, inliers, RANSAC, threshold).  With M good matches and
 * H = DLIOM_FEATURE_RANSAC_HYPOTHESES: if M (M - 1) / 2 <= H (M <= 63) the hypotheses are all pairs i < j in
 * lexicographic order; otherwise there are H, and hypothesis h draws
 *     z = seed + h;  z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31;                       (splitmix64, 64-bit wrap-around)
 *     i = (uint32)z % M;  j = (uint32)(z >> 32) % (M - 1);  j += (j >= i);
 * Every hypothesis is evaluated (no adaptive stop).  M < 2 has none.  With p = from, P = to:
 *     dx = p_j.x - p_i.x;  dy = p_j.y - p_i.y;  ex = P_j.x - P_i.x;  ey = P_j.y - P_i.y;
 *     den = dx * dx + dy * dy;                          den == 0: degenerate, the hypothesis scores -1
 *     a = (dx * ex + dy * ey) / den;  b = (dx * ey - dy * ex) / den;
 *     tx = P_i.x - (a * p_i.x - b * p_i.y);  ty = P_i.y - (b * p_i.x + a * p_i.y);
 * Match k is an inlier iff, with rx = ((a * p_k.x - b * p_k.y) + tx) - P_k.x and ry = ((b * p_k.x + a * p_k.y) + ty)
 * - P_k.y, rx * rx + ry * ry <= threshold * threshold.  The best hypothesis has the most inliers, ties to the lowest h;
 * all degenerate (or none): DLIOM_FEATURE_NO_MODEL.
 *
 * Refit over the best hypothesis's n inliers, the closed-form least-squares similarity (what OpenCV's LM refinement
 * converges to); every sum sequential in match order from 0.0:
 *     mpx = (sum p.x) / n, mpy, mPx, mPy likewise;  per inlier dcx = p.x - mpx, dcy = p.y - mpy, ecx = P.x - mPx, ecy = P.y - mPy;
 *     sdd += dcx * dcx + dcy * dcy;  sde += dcx * ecx + dcy * ecy;  sx += dcx * ecy - dcy * ecx;
 *     sdd == 0: the hypothesis's own (a, b, tx, ty) stand; else a = sde / sdd;  b = sx / sdd;
 *     tx = mPx - (a * mpx - b * mpy);  ty = mPy - (b * mpx + a * mpy).
 * On the host: scale = sqrt(a * a + b * b); |scale - 1| > scale_estimated_tolerance: DLIOM_FEATURE_SCALE_REJECTED
 * (:510-514); else DLIOM_FEATURE_MATCHED with theta = atan2(b, a) (:516-517) and the translation (tx, ty) (:519-525).
 *
 * No floating-point atomics anywhere: two calls on one input give the same bytes.  Malformed input fails the whole
 * call with DLIOM_ERR_INVALID_ARGUMENT before anything runs. */
#define DLIOM_FEATURE_RANSAC_HYPOTHESES 2000 /* OpenCV's default iteration cap */
#define DLIOM_FEATURE_MAX_GOOD 4096          /* good matches a pair (the RANSAC kernel keeps a pair's points in LDS) */
#define DLIOM_FEATURE_TRAIN_CHUNK 64         /* train descriptors staged in LDS at a time (feature_knn_kernel) */
#define DLIOM_FEATURE_MAX_TRAIN_SETS 8192    /* train keys of one dliom_feature_index_match call (the page-locked block) */
#define DLIOM_FEATURE_MAX_KEYPOINTS (1 << 20) /* key points of one set */
enum {
  DLIOM_FEATURE_MATCHED = 0,
  DLIOM_FEATURE_TOO_FEW_KEYPOINTS = 1,
  DLIOM_FEATURE_TOO_FEW_GOOD_MATCHES = 2,
  DLIOM_FEATURE_NO_MODEL = 3,
  DLIOM_FEATURE_SCALE_REJECTED = 4
};
typedef struct dliom_feature_index dliom_feature_index;
typedef struct dliom_feature_match_options {
  double good_match_ratio_of_distance;  /* constraint_builder_options.proto, as the fork reads them (:485-513) */
  int minimum_good_match_num;
  int reserved;                         /* 0 */
  double ransac_threshold;              /* ransac_thresh_of_2d_transform_estimate */
  double scale_estimated_tolerance;
  uint64_t seed;
} dliom_feature_match_options;
typedef struct dliom_submap_match {
  int64_t key;      /* the train key */
  int status;       /* DLIOM_FEATURE_*, or DLIOM_ERR_CAPACITY for this pair alone */
  int good_matches; /* 0 under TOO_FEW_KEYPOINTS */
  int inliers;      /* of the best hypothesis; 0 where no hypothesis was evaluated */
  int hypothesis;   /* its index h, -1 where there is none */
  double a, b, tx, ty; /* [a -b tx; b a ty]: query frame -> train frame; 0 where there is no model */
  double scale, theta;
} dliom_submap_match;
typedef struct dliom_feature_match_stats {
  int64_t pairs, matched, too_few_keypoints, too_few_good_matches, no_model, scale_rejected, over_capacity;
  int64_t ransac_pairs; /* pairs whose hypotheses were evaluated */
  int64_t read_backs;   /* polled read-backs of the call: 1, or 0 when no pair reached the device */
  /* milliseconds of the three kernels; filled (the call then synchronises the stream) only while the context's
   * profiling is on */
  double knn_ms, good_ms, ransac_ms;
} dliom_feature_match_stats;
typedef struct dliom_feature_ransac_result {
  int status;         /* DLIOM_FEATURE_MATCHED or DLIOM_FEATURE_NO_MODEL (no scale gate here: `scale` is reported) */
  int inliers;
  int hypothesis;
  int num_hypotheses; /* M (M - 1) / 2 or DLIOM_FEATURE_RANSAC_HYPOTHESES */
  double a, b, tx, ty, scale, theta;
} dliom_feature_ransac_result;
typedef struct dliom_feature_index_memory {
  int64_t sets, keypoints, descriptor_bytes, keypoint_bytes, scratch_bytes;
} dliom_feature_index_memory;
/* The descriptors and key points of all stored sets stay in HBM.  One thread at a time per index, like its context;
 * destroy the index before the context. */
int dliom_feature_index_create(dliom_ctx* ctx, int descriptor_size, dliom_feature_index** index);
void dliom_feature_index_destroy(dliom_feature_index* index);
int dliom_feature_index_size(const dliom_feature_index* index, int64_t* num_sets);
int dliom_feature_index_memory_stats(const dliom_feature_index* index, dliom_feature_index_memory* out);
/* descriptors: count x descriptor_size floats; keypoints_xy: count x 2 floats (cv::KeyPoint::pt, pixels); ox, oy: the
 * image's corner as ProjectToCvMat returns it; resolution: metres a pixel.  Refuses (DLIOM_ERR_INVALID_ARGUMENT) a
 * duplicate key, a non-finite value, count < 0 or > DLIOM_FEATURE_MAX_KEYPOINTS.  count 0 or 1 is stored and later
 * yields DLIOM_FEATURE_TOO_FEW_KEYPOINTS. */
int dliom_feature_index_add(dliom_feature_index* index, int64_t key, const float* descriptors, const float* keypoints_xy,
                            int32_t count, double ox, double oy, double resolution);
/* DeleteScanMatcher: an unknown key is DLIOM_ERR_INVALID_ARGUMENT. */
int dliom_feature_index_remove(dliom_feature_index* index, int64_t key);
/* The stored set `query_key` against each of train_keys[0 .. count): results[k] belongs to train_keys[k].  Three
 * launches and one polled read-back for the whole list.  An unknown key, count < 0, NULL options / results, a
 * non-finite or negative option: DLIOM_ERR_INVALID_ARGUMENT; count > DLIOM_FEATURE_MAX_TRAIN_SETS: DLIOM_ERR_TOO_LARGE;
 * all before anything runs.  stats may be NULL. */
int dliom_feature_index_match(dliom_feature_index* index, int64_t query_key, const int64_t* train_keys, int count,
                              const dliom_feature_match_options* options, dliom_submap_match* results,
                              dliom_feature_match_stats* stats);
/* Diagnostics for the tests, both on the device.  The two nearest neighbours of every key point of `query_key` in
 * `train_key` (both sets >= 2 key points, else DLIOM_ERR_INVALID_ARGUMENT): four arrays of the query's count. */
int dliom_feature_index_knn(dliom_feature_index* index, int64_t query_key, int64_t train_key, int32_t* j0, int32_t* j1,
                            float* d0, float* d1);
/* The hypotheses and the refit on M given matches (2 <= M <= DLIOM_FEATURE_MAX_GOOD; x y interleaved);
 * inlier_mask: M bytes of the best hypothesis's inliers (zeros under NO_MODEL), may be NULL. */
int dliom_feature_ransac(dliom_ctx* ctx, const float* from_xy, const float* to_xy, int num_matches, double threshold,
                         uint64_t seed, dliom_feature_ransac_result* result, unsigned char* inlier_mask);

/* ---- submap image features ----------------------------------------------------------------------
 * The first half of ConstraintBuilder3D::ExtractFeaturesForSubmap (constraint_builder_3d.cc:451-458): cv::threshold,
 * cv::erode and SURF::detectAndCompute on the image dliom_grid_project_to_image makes, so that loop detection runs from
 * a grid in HBM to `matched_submaps` without the image or the features leaving the device.
 * PARITY UNPINNED AGAINST OPENCV: OpenCV (and its non-free xfeatures2d) is neither in the reference tree nor a
 * dependency here, so its result cannot be pinned.  What is pinned, bit for bit against a CPU model (tests/cpp/surf_model.cc), is this definition:
 * SURF as OpenCV parametrises it (hessianThreshold 400, constraint_builder_3d.h:206; 4 octaves, 3 layers an octave, 64
 * dimensions, oriented).
 *
 * Arithmetic.  Every float operation is rounded on its own (no contraction), in the order written, parentheses first
 * and otherwise left to right.  round() is round-half-to-even (cvRound, rintf).  No transcendental function runs on
 * the device: the two Gaussian tables are made on the host when the library is loaded, with the C library's exp().
 * W, H: the image's width and height; pixels are bytes, row-major.
 *
 * (1) Binarise and erode (:451-455).  b(x, y) = 255 if pixel > binary_threshold else 0.  With k =
 * structure_element_size (1 <= k <= DLIOM_SURF_MAX_STRUCTURE_ELEMENT) and a = k / 2, e(x, y) = min of b(x + dx - a,
 * y + dy - a) over 0 <= dx, dy < k, positions outside the image taking no part.  k = 1 is the identity.  The projected
 * image's empty pixels are 224, above the reference's threshold of 200, hence white: that is the reference.
 *
 * (2) Integral image.  S is (H + 1) x (W + 1) 32-bit integers, S(x, y) = sum of e over [0, x) x [0, y); exact, so any
 * summation order gives it.  W * H > DLIOM_SURF_MAX_PIXELS (2^23; 2^23 * 255 < 2^31) is DLIOM_ERR_TOO_LARGE.  The sum
 * over a box with corners (x1, y1), (x2, y2) is S(x1, y1) + S(x2, y2) - S(x1, y2) - S(x2, y1) modulo 2^32, as an int.
 *
 * (3) Layers.  Octave o < n_octaves, layer l in [0, n_octave_layers + 1]: size = (9 + 6 l) << o, step = 1 << o.  A
 * template (DLIOM_SURF_TEMPLATE_*: rows of {x1, y1, x2, y2, weight} on a 9 x 9 pattern) is resized with ratio =
 * (float)size / 9.0f: every corner c becomes round(ratio * (float)c), and the box weight w = (float)weight /
 * (float)((x2 - x1) * (y2 - y1)) of the resized corners.  A template's response at (x0, y0) is r = 0.0f; r = r +
 * (float)(box sum at the corners shifted by (x0, y0)) * w, box after box in the table's order.  The layer's arrays det
 * and trace have H / step rows and W / step columns and hold 0.0f where there is no sample.  If size <= H and size <=
 * W the samples are i < 1 + (H - size) / step, j < 1 + (W - size) / step, taken at (x0, y0) = (j step, i step) and
 * stored at row i + m, column j + m, m = (size / 2) / step:
 *     det = dxx * dyy - (0.81f * dxy) * dxy;   trace = dxx + dyy.
 *
 * (4) Maxima, in the layers l = 1 .. n_octave_layers.  With margin = (size_{l+1} / 2) / step + 1, an array position
 * (i, j) with margin <= i < rows - margin, margin <= j < cols - margin is a candidate iff v = det_l(i, j) >
 * (float)hessian_threshold and v > each of its 26 neighbours N(s, r, c) = det_{l+s}(i + r, j + c).  Refinement, in
 * float:
 *     bx = -((N(0,0,1) - N(0,0,-1)) * 0.5f);  by = -((N(0,1,0) - N(0,-1,0)) * 0.5f);  bs = -((N(1,0,0) - N(-1,0,0)) * 0.5f);
 *     axx = (N(0,0,-1) - 2.0f * v) + N(0,0,1);  ayy = (N(0,-1,0) - 2.0f * v) + N(0,1,0);  ass = (N(-1,0,0) - 2.0f * v) + N(1,0,0);
 *     axy = (((N(0,1,1) - N(0,1,-1)) - N(0,-1,1)) + N(0,-1,-1)) * 0.25f;
 *     axs = (((N(1,0,1) - N(1,0,-1)) - N(-1,0,1)) + N(-1,0,-1)) * 0.25f;
 *     ays = (((N(1,1,0) - N(1,-1,0)) - N(-1,1,0)) + N(-1,-1,0)) * 0.25f;
 * then Cramer's rule in double on a = axx, b = axy, c = axs, d = ayy, e = ays, f = ass, p = bx, q = by, r = bs:
 *     c00 = d * f - e * e;  c01 = b * f - c * e;  c02 = b * e - c * d;  D = (a * c00 - b * c01) + c * c02;
 *     qfer = q * f - e * r;  qedr = q * e - d * r;  brqc = b * r - q * c;
 *     x0 = ((p * c00 - b * qfer) + c * qedr) / D;  x1 = ((a * qfer - p * c01) + c * brqc) / D;
 *     x2 = ((a * (d * r - q * e) - b * brqc) + p * c02) / D;
 * The candidate is kept iff D != 0 and, with (t0, t1, t2) = (float)(x0, x1, x2), not all t are 0 and every |t| <= 1.
 *     x = ((float)(step (j - m)) + (float)(size - 1) * 0.5f) + t0 * (float)step,   y likewise from i and t1,
 *     size = (float)round((float)size_l + t2 * (float)(size_l - size_{l-1})),
 *     response = v,  laplacian sign = (trace_l(i, j) > 0) - (trace_l(i, j) < 0),  angle = -1 until step 6.
 *
 * (5) Order.  By response descending; ties to the lowest generation index (o << 25 | l << 23 | i cols + j), which is
 * unique.  More than DLIOM_SURF_MAX_KEYPOINTS kept candidates: DLIOM_ERR_CAPACITY.
 *
 * (6) Orientation.  s = size * 1.2f / 9.0f; side = 2 round(2.0f * s).  H + 1 < side or W + 1 < side: the key point is
 * dropped.  The wavelets DLIOM_SURF_WAVELET_X / _Y (on a 4 x 4 pattern) are resized to `side` as in (3).  g = the
 * Gaussian table of 13 entries, sigma 2.5: t_n = exp(-(x_n * x_n) / (2.0 * sigma * sigma)) with x_n = n - (N - 1) * 0.5
 * in double, g_n = (float)(t_n / (t_0 + t_1 + ...)) summed in index order.  For i = -6 .. 6 (outer) and j = -6 .. 6
 * with i i + j j <= 36, the DLIOM_SURF_ORI_SAMPLES offsets:
 *     px = round((x + (float)i * s) - (float)(side - 1) / 2.0f);  py = round((y + (float)j * s) - (float)(side - 1) / 2.0f);
 * the sample is skipped unless 0 <= px < W + 1 - side and 0 <= py < H + 1 - side; else X = (response of wavelet X at
 * (px, py)) * (g[i + 6] * g[j + 6]), Y likewise, and A = round(fastAtan2(Y, X)).  No sample: dropped.  fastAtan2(y, x),
 * degrees, with p1, p3, p5, p7 = 0.9997878412794807f, -0.3258083974640975f, 0.1555786518463281f,
 * -0.04432655554792128f, each times (float)(180 / pi):
 *     c = min(|x|, |y|) / (max(|x|, |y|) + (float)DBL_EPSILON);  c2 = c * c;  a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
 *     |x| < |y|: a = 90.0f - a;  then x < 0: a = 180.0f - a;  then y < 0: a = 360.0f - a.
 * Windows w = 0, 5, .., 355: sumx, sumy start at 0.0f and take, sequentially in sample order, the X and Y of every
 * sample with d = |A - w| < 30 or d > 330.  The best window has the greatest sumx * sumx + sumy * sumy above 0, ties to
 * the lowest w; with n = sqrtf(bestx * bestx + besty * besty), n == 0 (also: no window above 0): dropped.
 * angle = fastAtan2(-besty, bestx); the descriptor's frame is cos = bestx / n, sin = besty / n.
 *
 * (7) Descriptor.  w = (int)(21.0f * s); off = -((float)(w - 1) / 2.0f); sx = (x + off * cos) + off * sin; sy = (y -
 * off * sin) + off * cos.  Window pixel (i, j), 0 <= i, j < w, is e at (round((sx + (float)i * sin) + (float)j * cos),
 * round((sy + (float)i * cos) - (float)j * sin)), each coordinate clamped to the image.  The 21 x 21 patch, exact in
 * integers: with ov(k, p) = min(21 k + 21, w (p + 1)) - max(21 k, w p) where positive, patch(pi, pj) = (2 sum + w w) /
 * (2 w w), sum = the sum over (ki, kj) of ov(ki, pi) ov(kj, pj) window(ki, kj).  h = the Gaussian table of 20 entries,
 * sigma 3.3.  For 0 <= i, j < 20:
 *     DX(i, j) = (float)(patch(i, j+1) - patch(i, j) + patch(i+1, j+1) - patch(i+1, j)) * (h[i] * h[j]);
 *     DY(i, j) = (float)(patch(i+1, j) - patch(i, j) + patch(i+1, j+1) - patch(i, j+1)) * (h[i] * h[j]).
 * Sub-region (a, b), 0 <= a, b < 4, holds rows 5a .. 5a+4 and columns 5b .. 5b+4; its four sums of DX, DY, |DX|, |DY|
 * start at 0.0f and run in row-major order; they are values 4 (4a + b) .. + 3 of the descriptor.  q = 0.0f; q = q +
 * v * v over the 64 values in order; every value is then multiplied by 1.0f / (sqrtf(q) + (float)DBL_EPSILON).
 *
 * (8) Dropped key points leave the list; the order of the rest is kept.
 *
 * (9) Options.  extended and upright are reserved: 0.  n_octaves in [1, 4], n_octave_layers in [1, 3],
 * hessian_threshold finite and >= 0, binary_threshold in [0, 255], structure_element_size as in (1); anything else is
 * DLIOM_ERR_INVALID_ARGUMENT.
 *
 * No floating-point atomics anywhere: two calls on one input give the same bytes. */
#define DLIOM_SURF_MAX_PIXELS (1 << 23)
#define DLIOM_SURF_MAX_KEYPOINTS 65536
#define DLIOM_SURF_MAX_STRUCTURE_ELEMENT 33
#define DLIOM_SURF_DESCRIPTOR_SIZE 64
#define DLIOM_SURF_KEYPOINT_FLOATS 7 /* x, y, size, angle, response, octave, laplacian sign */
#define DLIOM_SURF_SIZE0 9
#define DLIOM_SURF_SIZE_INCREMENT 6
#define DLIOM_SURF_ORI_RADIUS 6
#define DLIOM_SURF_ORI_SAMPLES 113 /* offsets with i i + j j <= 36 */
#define DLIOM_SURF_ORI_SIGMA 2.5
#define DLIOM_SURF_PATCH 20
#define DLIOM_SURF_DESCRIPTOR_SIGMA 3.3
#define DLIOM_SURF_TEMPLATE_DXX {{0, 2, 3, 7, 1}, {3, 2, 6, 7, -2}, {6, 2, 9, 7, 1}}
#define DLIOM_SURF_TEMPLATE_DYY {{2, 0, 7, 3, 1}, {2, 3, 7, 6, -2}, {2, 6, 7, 9, 1}}
#define DLIOM_SURF_TEMPLATE_DXY {{1, 1, 4, 4, 1}, {5, 1, 8, 4, -1}, {1, 5, 4, 8, -1}, {5, 5, 8, 8, 1}}
#define DLIOM_SURF_WAVELET_X {{0, 0, 2, 4, -1}, {2, 0, 4, 4, 1}}
#define DLIOM_SURF_WAVELET_Y {{0, 0, 4, 2, 1}, {0, 2, 4, 4, -1}}
typedef struct dliom_surf_options {
  int binary_threshold;       /* cv_binary_threshold (pose_graph.lua:27: 200) */
  int structure_element_size; /* cv_structure_element_size (pose_graph.lua:28: 3) */
  double hessian_threshold;   /* 400 */
  int n_octaves, n_octave_layers, extended, upright; /* 4, 3, 0, 0 */
} dliom_surf_options;
dliom_surf_options dliom_surf_default_options(void);
/* Step 1 alone: host bytes in and out (width * height each).  width or height 0 is DLIOM_OK and writes nothing. */
int dliom_image_binarize_erode(dliom_ctx* ctx, const uint8_t* image, int32_t width, int32_t height,
                               const dliom_surf_options* options, uint8_t* out);
/* Diagnostic for the tests: steps 2 and 3 for one layer on an image taken as it is (no step 1).  octave in [0, 3],
 * layer in [0, 4].  *rows, *cols: the arrays' size; det and trace (rows * cols floats each) may both be NULL for the
 * size alone. */
int dliom_surf_layer(dliom_ctx* ctx, const uint8_t* image, int32_t width, int32_t height, int octave, int layer, float* det,
                     float* trace, int32_t* rows, int32_t* cols);
/* Steps 1-8 on a caller's image.  keypoints: DLIOM_SURF_KEYPOINT_FLOATS floats a key point; descriptors:
 * DLIOM_SURF_DESCRIPTOR_SIZE floats a key point; capacity: key points the buffers hold.  *count = the key points
 * found; keypoints == NULL and descriptors == NULL asks for the count alone; *count > capacity is DLIOM_ERR_CAPACITY
 * (nothing written).  More than DLIOM_SURF_MAX_KEYPOINTS candidates (step 5) is DLIOM_ERR_CAPACITY whatever the
 * capacity, with *count = the candidates. */
int dliom_surf_detect_and_compute(dliom_ctx* ctx, const uint8_t* image, int32_t width, int32_t height,
                                  const dliom_surf_options* options, float* keypoints, float* descriptors, int32_t capacity,
                                  int32_t* count);
/* ExtractFeaturesForSubmap's first half into the index: project `grid` (dliom_grid_project_to_image), then steps 1-8,
 * and store the set under `key` with the key points' (x, y) -- neither the image nor the features leave HBM.  The
 * stored set equals dliom_grid_project_to_image -> dliom_surf_detect_and_compute -> dliom_feature_index_add bit for
 * bit.  The index must have descriptor size 64 and share the grid's context.  An empty projection (0 x 0) or an image
 * too small for any layer stores an empty set (later DLIOM_FEATURE_TOO_FEW_KEYPOINTS, as :476-483).  count, ox, oy,
 * resolution (each may be NULL): the set's size and the image's corner and metres a pixel.  DLIOM_ERR_CAPACITY: a
 * projection above DLIOM_XRAY_MAX_PIXELS, or more than DLIOM_SURF_MAX_KEYPOINTS candidates; DLIOM_ERR_TOO_LARGE: an image
 * above DLIOM_SURF_MAX_PIXELS; DLIOM_ERR_INVALID_ARGUMENT: a NULL argument, a duplicate key, another descriptor size or
 * context, refused options.  On every error nothing is stored and count, ox, oy, resolution are not written. */
int dliom_feature_index_add_from_grid(dliom_feature_index* index, int64_t key, const dliom_grid* grid,
                                      const double transform7[7], const dliom_surf_options* options, int32_t* count, double* ox,
                                      double* oy, double* resolution);

/* ---- painting submap slices into one map (io/submap_painter.cc:30-108, cartographer_ros msg_conversion.cc:321-368) ----
 * io::PaintSubmapSlices draws every submap's X-ray texture into one ARGB32 image with cairo, and CreateOccupancyGridMsg
 * turns that image into the /map occupancy grid.  Here the textures stay in HBM (dliom_submap_slice) and one gather
 * kernel composites them: every output pixel is produced by one thread, samples every slice that can reach it once, in
 * the order given, and is written once.  cairo is not a dependency, so the problem is stated here, once; the device
 * equals a CPU model of this statement (tests/submap_painter_common.py) bit for bit, and the statement is checked against
 * the system's cairo where there is one (tests/test_submap_painter_host.py).  The sampling below is pixman's bilinear
 * filter, which is what cairo's default CAIRO_FILTER_GOOD uses whenever the map's resolution is no coarser than the
 * slices' (0.05 m against 0.10 m, the occupancy grid node's default with 3D submaps): there the statement gives what the
 * reference shows, up to cairo's own 16.16 rounding of the matrix (a few levels in red and green).  For a map coarser than
 * a slice cairo >= 1.14 switches to a box-convolution filter: the statement stays bilinear, parity unpinned against cairo.
 * cairo's trajectory drawing and PNG output stay out of scope: parity unpinned against cairo there too, nothing is built.
 *
 * The statement.  Integer or ordered double arithmetic throughout (-ffp-contract=off), no transcendental function.
 *  Texel      a slice is height x width (intensity, alpha) byte pairs as dliom_grid_xray_texture emits them; the texel is
 *             alpha << 24 | intensity << 16 | observed << 8 with observed = (intensity == 0 && alpha == 0) ? 0 : 255
 *             (DrawTexture, submap_painter.cc:158-177).  A fetch outside the slice is 0.
 *  Matrices   doubles.  P = pose * slice_pose (the Rigid3d product: t = pose.q * slice_pose.t + pose.t, q = normalized
 *             quaternion product); with q = (w, x, y, z) of P and tx = 2x, ty = 2y, tz = 2z:
 *               r00 = 1 - (ty*y + tz*z), r01 = ty*x - tz*w, r10 = ty*x + tz*w, r11 = 1 - (tx*x + tz*z)
 *             m = (xx, yx, xy, yy, x0, y0) = (r10, r00, -r11, -r01, P.t[0], -P.t[1]) in cairo's convention
 *             x' = xx*x + xy*y + x0, y' = yx*x + yy*y + y0.  With k = 1. / resolution and s = the slice's resolution the
 *             slice's matrix Scale(s), then m, then Scale(k) -- cairo_matrix_multiply with its zero terms dropped -- is
 *               L = ((m.xx*k)*s, (m.yx*k)*s, (m.xy*k)*s, (m.yy*k)*s, m.x0*k, m.y0*k)
 *  Layout     the corners (0,0), (w,0), (0,h), (w,h) of every slice through L, (xx*x + xy*y) + x0 and (yx*x + yy*y) + y0,
 *             each rounded to float; min and max over all slices in float; per axis size = int(ceil(max - min)) + 10 with
 *             the difference in float, origin = -min + 5.f in float (kPaddingPixel = 5).  A slice with w == 0 or h == 0
 *             contributes its corners like any other (one point when both are 0) and paints nothing.
 *  Inverse    F = L with x0 + origin[0], y0 + origin[1] (double sums).  det = F.xx*F.yy - F.yx*F.xy and
 *               ixx = F.yy/det, ixy = -F.xy/det, ix0 = (F.xy*F.y0 - F.yy*F.x0)/det
 *               iyx = -F.yx/det, iyy = F.xx/det, iy0 = (F.yx*F.x0 - F.xx*F.y0)/det
 *             A, B, E = rint(ixx * 2^32), rint(ixy * 2^32), rint(ix0 * 2^32) as int64 (round half to even), C, D, G
 *             likewise from the second row: 32.32 fixed point.
 *  Bound      refused with DLIOM_ERR_TOO_LARGE unless all six are finite, |ixx|, |ixy|, |iyx|, |iyy| <= 2^10 (texels a
 *             pixel) and |ixx|*width + |ixy|*height + |ix0| + 1 < 2^29, likewise the second row (doubles, in this order).
 *             Then |A x + B y + E + ((A + B) >> 1) - 2^31| < 2^61 + 2^33 for every pixel 0 <= x < width, 0 <= y < height
 *             -- the sum of the magnitudes is below 2^29 texels = 2^61, each rint moves a term by at most x/2, y/2 or 1/2
 *             units with x, y < 2^23 (width * height <= 2^26 and both >= 10) -- so U and V fit an int64 with room and
 *             x1, y1 fit an int32.
 *  Sample     pixel (x, y): U = A*x + B*y + E + ((A + B) >> 1) - 2^31 (arithmetic shifts; the pixel's centre in texel
 *             centres), V likewise from C, D, G.  x1 = U >> 32, dx = ((U >> 25) & 127) << 1, y1 and dy likewise (pixman's
 *             seven-bit weights).  w_br = dx*dy, w_tr = (dx << 8) - w_br, w_bl = (dy << 8) - w_br,
 *             w_tl = 65536 - (dx << 8) - (dy << 8) + w_br; tl, tr, bl, br = the texels at (x1, y1), (x1 + 1, y1),
 *             (x1, y1 + 1), (x1 + 1, y1 + 1); each of the four channels is (tl*w_tl + tr*w_tr + bl*w_bl + br*w_br) >> 16.
 *  Composite  the map starts as 0xFF800000; slices are painted in the order given; per channel
 *             d = min(255, s + MUL8(d, 255 - s_alpha)), MUL8(a, b): t = a*b + 128; ((t >> 8) + t) >> 8.  The saturation
 *             matters: the texel is not premultiplied, intensity can exceed alpha.
 *  Grid       occupancy row r is image row height - 1 - r; value = -1 if the green byte is 0, else table[red] with
 *             table[c] = lround((1. - c / 255.) * 100.) in double (dliom_submap_occupancy_table).
 *             origin_xy[0] = -double(origin[0]) * resolution; origin_xy[1] = double(float(-height) + origin[1]) *
 *             resolution: the sum in float, as C++ evaluates the reference's int + float.
 *
 * Sizes: pixels / data == NULL is a size query (DLIOM_OK, sizes and origin filled); capacity counts pixels (cells); a
 * buffer smaller than the map fills the sizes and returns DLIOM_ERR_CAPACITY; more than DLIOM_XRAY_MAX_PIXELS pixels fills
 * the sizes and returns DLIOM_ERR_CAPACITY whatever the buffer.  DLIOM_ERR_INVALID_ARGUMENT: no slices, a NULL pointer,
 * a resolution or pose entry that is not finite, a resolution <= 0, a negative slice size, slices of another context.
 * DLIOM_ERR_TOO_LARGE: the bound above, a corner that is not finite as float, a size beyond int32, a slice of more than
 * DLIOM_XRAY_MAX_PIXELS texels, more than DLIOM_SUBMAP_PAINTER_MAX_SLICES slices or more than
 * DLIOM_SUBMAP_PAINTER_MAX_PAIRS (tile, slice) pairs in one paint. */
#define DLIOM_SUBMAP_PAINTER_TILE 16                       /* the paint kernel's workgroup covers 16 x 16 pixels */
#define DLIOM_SUBMAP_PAINTER_MAX_PAIRS (INT64_C(1) << 30)  /* 4 bytes each in the tile lists */
#define DLIOM_SUBMAP_PAINTER_MAX_SLICES (1 << 24)
typedef struct dliom_submap_slice dliom_submap_slice;
typedef struct dliom_submap_slice_description {
  int32_t width, height; /* texels */
  double resolution;     /* metres a texel */
  double slice_pose7[7]; /* SubmapSlice::slice_pose */
  double pose7[7];       /* SubmapSlice::pose, the submap's global pose */
} dliom_submap_slice_description;
typedef struct dliom_submap_painter_stats {
  int64_t launches;         /* kernel launches of the context's last paint: the same whatever the number of slices */
  int64_t texels_uploaded;  /* host -> device texels of dliom_submap_slice_create since the context was created */
  int64_t tile_slice_pairs; /* (tile, slice) pairs the last paint's lists held */
} dliom_submap_painter_stats;
/* Uploads height * width (intensity, alpha) byte pairs once; they stay in HBM until the slice is destroyed.  cells may be
 * NULL when width * height == 0. */
int dliom_submap_slice_create(dliom_ctx* ctx, const uint8_t* cells, int32_t width, int32_t height, double resolution,
                              const double slice_pose7[7], const double pose7[7], dliom_submap_slice** out);
/* FillSubmapSlice for a device grid: dliom_grid_xray_texture's kernels, the texture kept on the device (only the
 * bounding-box read-back that sizes it remains).  pose = global_submap_pose; the slice is on the grid's context. */
int dliom_submap_slice_create_from_grid(const dliom_grid* grid, const double global_submap_pose7[7], dliom_submap_slice** out);
/* The slice's new global pose after an optimisation.  Host only: no texture data moves. */
int dliom_submap_slice_set_pose(dliom_submap_slice* slice, const double pose7[7]);
int dliom_submap_slice_info(const dliom_submap_slice* slice, dliom_submap_slice_description* out);
int dliom_submap_slice_destroy(dliom_submap_slice* slice);
/* Layout and Inverse of the statement on the host, from plain descriptions: no device, no context.  fixed6 (may be NULL):
 * A, B, E, C, D, G per slice, n * 6 values; written only when the call returns DLIOM_OK. */
int dliom_submap_slices_layout(const dliom_submap_slice_description* slices, int64_t n, double resolution, int32_t* width,
                               int32_t* height, float origin2f[2], int64_t* fixed6);
int dliom_submap_occupancy_table(int8_t table256[256]);
/* PaintSubmapSlices: pixels = height * width words alpha << 24 | red << 16 | green << 8 | blue, row-major
 * (CAIRO_FORMAT_ARGB32 on a little-endian host).  Runs on the context's stream and synchronises it.  ctx == NULL stands
 * for the context the slices were created on (they must all share one). */
int dliom_submap_slices_paint(dliom_ctx* ctx, const dliom_submap_slice* const* slices, int64_t n, double resolution,
                              uint32_t* pixels, int64_t capacity, int32_t* width, int32_t* height, float origin2f[2]);
/* PaintSubmapSlices + CreateOccupancyGridMsg's data and origin: painted and converted on the device, one byte a cell
 * comes back.  origin2f may be NULL. */
int dliom_submap_slices_occupancy(dliom_ctx* ctx, const dliom_submap_slice* const* slices, int64_t n, double resolution,
                                  int8_t* data, int64_t capacity, int32_t* width, int32_t* height, float origin2f[2],
                                  double origin_xy[2]);
int dliom_ctx_submap_painter_stats(const dliom_ctx* ctx, dliom_submap_painter_stats* out);

/* Per-context choices a caller may make; none of them changes a result (every kernel variant is parity-tested).  The
 * library never reads the environment (tuning experiments live in `make experiments` builds only). */
enum {
  DLIOM_TUNE_SCORE_KERNEL = 0,        /* RTCSM3D score volume: 3 LDS-box kernel over the dense mirror when the search suits
                                         it (default), 2 rotation-per-lane over the dense mirror, 1 rotation-per-lane over
                                         the leaf table, 0 point-per-lane over the leaf table */
  DLIOM_TUNE_CSM_ONE_LAUNCH_MAX = 1,  /* CeresScanMatcher3D: clouds up to this many points (sum over grids) run the whole
                                         trust-region loop in one launch (default 4096, 0 = never) */
  DLIOM_TUNE_RESERVED_TEST_HOOK = 2,  /* reserved: dliom_ctx_set_tuning refuses it (DLIOM_ERR_INVALID_ARGUMENT).  Only a
                                         test build of the library (-DDLIOM_TEST_HOOKS, `make hooks` ->
                                         libdliom_hooks.so, loaded by one GPU test) accepts it: the next match then
                                         treats the box kernel's consistency word as set and takes the "redo on the
                                         dense kernel" path once; 2 / 3 force the de-skew check's overflow and fix
                                         paths, 4 / 5 the batch assembler's (every point recorded / the device's
                                         rotation also perturbed).  The shipped library contains no fault injection. */
  DLIOM_TUNE_COUNT = 3
};
int dliom_ctx_set_tuning(dliom_ctx* ctx, int knob, int value);
int dliom_ctx_get_tuning(const dliom_ctx* ctx, int knob, int* value);
/* Read-backs end in a completion word in coherent pinned host memory that the host polls (150 us), falling back to
 * hipStreamSynchronize: *count = how often that fallback was taken on this context.  A long kernel in front of a
 * read-back takes it legitimately; a count that grows with every call means the polling is not seeing the device's
 * writes (10x the latency, same results). */
int dliom_ctx_poll_fallbacks(const dliom_ctx* ctx, int64_t* count);
/* *count = polled read-backs on this context so far: the host round trips a caller's chain costs (a W-ref scan of the
 * front end: 8, profiles/r5_wref_full.json `read_backs_per_scan`). */
int dliom_ctx_read_backs(const dliom_ctx* ctx, int64_t* count);
/* *count = stream synchronisations the loop-closure paths made on this context so far (fast search, CeresScanMatcher3D,
 * dliom_cloud_create): with dliom_ctx_read_backs, the host round trips of a chain of such calls. */
int dliom_ctx_synchronizations(const dliom_ctx* ctx, int64_t* count);
/* The device voxel filter (sensor/internal/voxel_filter.cc:81-131) keeps "voxel -> first point" in a hash table whose
 * entries pack the voxel index (13 bits per axis) and the point index (24 bits) into one word, so that a voxel costs
 * one atomic.  A cloud with a point farther than 4095 voxel edges from the origin (61 m at 1.5 cm) does not fit: the
 * launch is repeated with 21-bit keys (same result).  *count = how often that happened on this context. */
int dliom_ctx_voxel_filter_reruns(const dliom_ctx* ctx, int64_t* count);
/* Page-locks a host buffer the caller keeps (a LiDAR driver's ring of scan buffers, the vector a
 * sensor::TimedPointCloudData is filled into): uploads from it -- dliom_add_range_data's scan, dliom_cloud_create's
 * points -- are then one asynchronous DMA instead of the runtime's staged copy of pageable memory (a 64 x 1024 scan of
 * 1 MB: ~38 us of a 0.55 ms W-ref scan, tools/wref_cpp.py --pinned-scans).  Registering costs hundreds of microseconds:
 * for buffers that live across scans, not per call.  Results do not depend on it.  Every entry point that takes such a
 * buffer has consumed it when it returns, pinned or not.  The reference has no counterpart (its data never leaves the host). */
int dliom_host_register(dliom_ctx* ctx, void* buffer, size_t bytes);
int dliom_host_unregister(dliom_ctx* ctx, void* buffer);

/* ---- PointCloud2 messages decoded on the device (cartographer_ros/sensor_bridge.cc:176-240, 286-299 and
 * msg_conversion.cc:185-226) ----
 * The per-point code in front of both pipelines: SensorBridge::HandlePointCloud2Message's four sensor branches with
 * HandleRangefinder's change of frame, and the export's ToPointCloudWithIntensities / ...RsLiDAR.  PCL and ROS are not
 * part of the reference tree this library is checked against, so this section is PARITY UNPINNED AGAINST PCL: the
 * statement below defines the result, and the device equals a CPU model of the statement bit for bit
 * (tests/point_cloud2_common.py, tests/cpp/point_cloud2_model.cc).
 *
 * The message is sensor_msgs/PointCloud2 as a plain struct.  Point i lies at
 *     data + (i / width) * row_step + (i % width) * point_step,      n = height * width points,
 * and a field of the table is `count` values of `datatype` (ROS's codes) at `offset` inside the point's record.
 * Fields are matched by name, the first of that name, as pcl::fromROSMsg does; nothing needs to be aligned.
 *
 * Modes, and where each takes the point time t and the intensity from (x, y, z: FLOAT32, count 1, in every mode):
 *   SLAM_OUSTER    (sensor_bridge.cc:183-194)  field "t", UINT32 [ns]
 *       rel_time_last = double(float(t_last) * 1e-9f)     the uint32 rounds to the nearest float, then a float product
 *       t_i = float(double(float(t_i) * 1e-9f) - rel_time_last)         the product is never fused with the subtraction
 *   SLAM_VELODYNE  (:195-208)  field "time", FLOAT32 [s]
 *       rel_time_last = double(time_last),   t_i = float(double(time_i) - rel_time_last)
 *   SLAM_ROBOSENSE (:209-225)  field "timestamp", FLOAT64 [s]
 *       t_i = float(timestamp_i - timestamp_last), subtracted in double
 *   SLAM_OTHER     (:226-235)  t = 0
 *   EXPORT         (msg_conversion.cc:187-210)  t = 0; intensity = the FLOAT32 field "intensity", or 1.0f for every point
 *                  when no field has that name
 *   EXPORT_RSLIDAR (:214-226)  t = 0; intensity = float(the UINT8 field "intensity")
 * `last` is the message's last point, whether or not it is kept.  The four SLAM modes drop a point when any of x, y, z
 * is NaN or +-Inf and keep the message's order; the export modes keep every point.
 *
 * *time = FromRos(stamp) = (stamp_sec + 719162 * 86400) * 10^7 + (stamp_nsec + 50) / 100, and for Ouster and Velodyne
 * plus FromSeconds(rel_time_last) = int64(rel_time_last * 1e7), truncated.
 *
 * Frame change (HandleRangefinder): with sensor_to_tracking = [tx, ty, tz, qw, qx, qy, qz] given, every kept point becomes
 * sensor_to_tracking.cast<float>() * p in float (Eigen's _transformVector order; the quaternion is cast as it is, not
 * normalised), t untouched, and origin = the cast translation.  NULL: the points stay in the sensor frame and origin is
 * zero -- the export applies its transform later, in the assembler.  (A non-finite coordinate an export mode keeps is a
 * copy of the message's bits only without a frame change: what arithmetic makes of a NaN or an infinity is a NaN whose
 * sign and payload are the machine's.)
 *
 * Refused with DLIOM_ERR_INVALID_ARGUMENT before anything touches a device (the host-only _check below answers the same):
 *   is_bigendian != 0;  a datatype outside 1 .. 8;  a field with offset + size * count > point_step;
 *   a required field that is missing, has another datatype or count != 1;  in the export modes an "intensity" field of
 *   another datatype or count (PCL would leave the point's default there: refused here instead of guessed);
 *   width * point_step > row_step;  height * row_step > data_size;  n >= 2^27;
 *   n == 0 in the three timed modes (the reference calls back() on an empty vector);
 *   a rel_time_last (Robosense: timestamp_last) that is not finite, or whose ticks do not fit an int64.
 * Found on the device and refused from the call's ONE read-back, leaving no object: a kept point whose t is not finite or
 * has |t * 1e7| >= 2^63 (the assembler's own rule for its input).
 *
 * A dliom_timed_cloud holds the kept points as packed (x, y, z, t) in HBM and, in the export modes, one intensity a
 * point, in a block of the cloud pool (handed back by _destroy after a whole-device synchronise, like a cloud's).  The
 * message's bytes are uploaded once -- from a buffer registered with dliom_host_register without a staging copy -- and
 * one pass gathers the fields, tests, computes t, changes the frame and compacts; the result never comes back unless
 * _download asks.  *out is an empty object, not NULL, when nothing is kept.  The message is free when the call returns. */
enum {
  DLIOM_POINT_FIELD_INT8 = 1,
  DLIOM_POINT_FIELD_UINT8 = 2,
  DLIOM_POINT_FIELD_INT16 = 3,
  DLIOM_POINT_FIELD_UINT16 = 4,
  DLIOM_POINT_FIELD_INT32 = 5,
  DLIOM_POINT_FIELD_UINT32 = 6,
  DLIOM_POINT_FIELD_FLOAT32 = 7,
  DLIOM_POINT_FIELD_FLOAT64 = 8
};
typedef struct {
  const char* name;
  uint32_t offset;
  uint32_t datatype; /* DLIOM_POINT_FIELD_* */
  uint32_t count;
} dliom_point_field;
typedef struct {
  uint32_t height, width, point_step, row_step;
  uint32_t is_bigendian;
  int32_t num_fields;
  const dliom_point_field* fields;
  const uint8_t* data;
  uint64_t data_size;
  uint32_t stamp_sec, stamp_nsec; /* header.stamp */
} dliom_point_cloud2;
typedef enum {
  DLIOM_POINT_CLOUD2_SLAM_OUSTER = 0,
  DLIOM_POINT_CLOUD2_SLAM_VELODYNE = 1,
  DLIOM_POINT_CLOUD2_SLAM_ROBOSENSE = 2,
  DLIOM_POINT_CLOUD2_SLAM_OTHER = 3,
  DLIOM_POINT_CLOUD2_EXPORT = 4,
  DLIOM_POINT_CLOUD2_EXPORT_RSLIDAR = 5
} dliom_point_cloud2_mode;
typedef struct dliom_timed_cloud dliom_timed_cloud;
/* Host only, no context: the refusals above; *time (may be NULL) and *rel_time_last (may be NULL; 0 in the untimed modes)
 * as the decode would return and use them. */
int dliom_point_cloud2_check(const dliom_point_cloud2* message, int mode, int64_t* time, double* rel_time_last);
int dliom_point_cloud2_decode(dliom_ctx* ctx, const dliom_point_cloud2* message, int mode, const double sensor_to_tracking[7],
                              dliom_timed_cloud** out, int64_t* time, float origin[3]);
int dliom_timed_cloud_destroy(dliom_timed_cloud* cloud);
int dliom_timed_cloud_size(const dliom_timed_cloud* cloud, int64_t* n);
int dliom_timed_cloud_has_intensities(const dliom_timed_cloud* cloud, int* has);
/* t of the first and of the last kept point, known on the host from the decode's read-back (both 0 for an empty object):
 * what HandleLaserScan's and AddRangeData's checks on the message need without a download. */
int dliom_timed_cloud_front_back_time(const dliom_timed_cloud* cloud, float* front, float* back);
/* xyzt: 4 n floats, intensities: n floats; either may be NULL.  Intensities the object does not have are refused. */
int dliom_timed_cloud_download(const dliom_timed_cloud* cloud, float* xyzt, float* intensities);
/* dliom_add_range_data with ranges_xyzt replaced by a decoded message: the raw points and the first range's time come
 * from the object, which stays the caller's; everything else, every result and the read-back count are that call's. */
int dliom_add_range_data_timed_cloud(dliom_ctx* ctx, const double prev_pose[7], const double predicted_pose[7],
                                     double scan_period, const dliom_timed_cloud* ranges, const float origin[3],
                                     float min_range, float max_range, float voxel_filter_size,
                                     dliom_cloud** returns_in_tracking, float origin_in_tracking[3], float current_pose[7]);
/* dliom_points_batch_from_sensor_points with points_xyzt and intensities replaced by a decoded message (an object
 * without intensities gives a batch without).  The points the exactness check records are fetched from the object. */
int dliom_points_batch_from_timed_cloud(dliom_ctx* ctx, dliom_trajectory* trajectory, int64_t cloud_time,
                                        const dliom_timed_cloud* points, const double sensor_to_tracking[7],
                                        dliom_points_batch** out);

/* ---- Two range sensors' clouds merged on the device (mapping/internal/3d/range_data_synchronizer.cc:29-130) ----
 * The RangeDataSynchronizer's per-point work on decoded messages, so that a second lidar, manual de-skew and accumulation
 * keep the ranges in HBM.  Which cloud is pending, when one is dropped as too old, "the secondary lidar may be too fast" and
 * the pass-through stay the caller's (cpp/dliom_cartographer.h): they need only stamps and first times, which the objects
 * carry.  The statement below defines the result; the device equals a CPU model of it (tests/range_sync_common.py) and the
 * adapter's host class bit for bit, in the same point order.
 *
 * Seconds(time) = double((time - 719162 * 86400 * 10^7) * 100) * 1e-9: common::ToSecondsStamp of universal-time ticks,
 * the subtraction and the product in int64.
 *
 * _stamp: StampRangeData (:115-130).  n < 2: a copy.  Otherwise
 *       t_i = float(-scan_period + double(i) * (scan_period / double(n - 1)))    the product is never fused with the sum
 *   and the last point's t = 0; x, y, z are copied.  First and last t are known on the host without a read-back.
 *
 * _merge: the branch at :69-111.  `primary` is the prior lidar's cloud, stamped primary_time; `primary_for_times` its
 * stamped copy under manual de-skew (same size) and NULL otherwise; `secondary` the pending cloud of the other lidar.
 *   current_end   = Seconds(primary_time)
 *   current_start = current_end + double(t of the first point of primary_for_times, or of primary when that is NULL),
 *                   current_end for an empty primary
 *   st            = Seconds(secondary_time)
 *   i_start       = the first i with current_start <= st + double(t_i) <= current_end, both bounds inclusive
 *   i_end + 1     = the first i > i_start with st + double(t_i) > current_end, or the secondary's size if there is none
 * The merged array is every point of `primary` as it is -- under manual de-skew with its UNSTAMPED t, as :94 takes them --
 * with origin index 0, then the secondary's points i_start .. i_end with origin index 1 and
 *       t = float((double(t_i) + st) - current_end),
 * and the result is that array in the order libstdc++'s std::sort leaves it in when it compares by t alone: where times
 * are equal (an Ouster column holds 64 or 128 of them) the order is what introsort's partitions make of it, and it decides
 * which point of a voxel AddRangeData's first filter keeps.  *out holds the points and the origin-index channel, one float
 * a point; its first and last t are known on the host.
 * Refused, leaving no object and the context usable: no i_start (the reference's CHECK at :84; also an empty secondary)
 * with DLIOM_ERR_INVALID_ARGUMENT; an arrangement of equal times the sort's replay refuses (dliom_diag_std_sort_order: its
 * work-list cap, the heap-sort fallback of a large segment) or more than 2^22 merged points with DLIOM_ERR_CAPACITY --
 * the caller then merges that scan on the host.  Inputs must be this context's and carry neither intensities nor the
 * origin-index channel.  Two read-backs a merge: the overlap's bounds, then the sort's status with the first and last t.
 *
 * An object with the channel is input to dliom_range_accumulator_add_timed_cloud only: dliom_add_range_data_timed_cloud
 * and dliom_points_batch_from_timed_cloud refuse it with DLIOM_ERR_INVALID_ARGUMENT. */
int dliom_timed_cloud_has_origin_index(const dliom_timed_cloud* cloud, int* has);
/* origin_index: n floats.  An object without the channel is refused. */
int dliom_timed_cloud_download_origin_index(const dliom_timed_cloud* cloud, float* origin_index);
int dliom_timed_cloud_stamp(dliom_ctx* ctx, const dliom_timed_cloud* in, double scan_period, dliom_timed_cloud** out);
int dliom_timed_clouds_merge(dliom_ctx* ctx, const dliom_timed_cloud* primary, const dliom_timed_cloud* primary_for_times,
                             int64_t primary_time, const dliom_timed_cloud* secondary, int64_t secondary_time,
                             dliom_timed_cloud** out);
/* cvtPointCloud (local_trajectory_builder_3d.cc): the xyz of a device object -- a decoded message, a stamped cloud or a
 * merge's result -- as a cloud of the context, in the object's order: a device copy, no de-skew, no filter.  The times and
 * the other channels are left behind.  One read-back (the cloud's bound). */
int dliom_timed_cloud_points(dliom_ctx* ctx, const dliom_timed_cloud* in, dliom_cloud** out);
/* dliom_range_accumulator_add with ranges_xyzt, origin_index and n taken from a device object -- a decoded message
 * (origin index 0 throughout) or a merge's result; `origins` stays the caller's table.  Results, read-back count and
 * refusals are those of the host-input call. */
int dliom_range_accumulator_add_timed_cloud(dliom_range_accumulator* accumulator, const double prev_pose[7],
                                            const double predicted_pose[7], double scan_period, const dliom_timed_cloud* ranges,
                                            const float* origins, int num_origins, float min_range, float max_range,
                                            float voxel_filter_size, float current_pose[7], int* num_accumulated);

/* ---- scan alignment by ICP, exact nearest neighbours ------------------------------------------------
 * gen_ground_truth_by_ndt_match.cc's default method (`icp`, :62): pcl::IterativeClosestPoint on two raw scans (:190-205:
 * 30 m correspondence distance, 100 iterations, both epsilons 1e-6, no RANSAC); LocalTrajectoryBuilder3D::MatchByICP
 * (local_trajectory_builder_3d.cc:937-967) carries the same settings with 3 m.  PARITY UNPINNED AGAINST PCL: PCL is
 * neither in the reference tree nor a dependency here.  What is pinned, bit for bit against a CPU model
 * (tests/icp_common.py), is this definition, our reading of PCL 1.8's IterativeClosestPoint, TransformationEstimationSVD
 * and DefaultConvergenceCriteria; where it differs from PCL, this text governs.
 *
 * Arithmetic.  Every operation is rounded on its own (no contraction), in the order written, parentheses first and
 * otherwise left to right.
 *
 * Points.  Source and target are clouds of float xyz (dliom_cloud); indices are those of the clouds as given.  A target point
 * with a non-finite coordinate is never a neighbour; a source point with a non-finite coordinate never has a
 * correspondence.
 *
 * Nearest neighbour.  For query p and target t_j, in float: dx = p.x - t.x, dy, dz likewise; d2 = (dx*dx + dy*dy) + dz*dz.
 * The neighbour is the j with the least d2 among the finite targets, ties (a d2 that overflowed to +inf included) to
 * the lowest j.  A correspondence exists iff (double)d2 <= D * D in double, D = the correspondence distance, inclusive;
 * D = +inf is "no bound".  The search is EXACT: the cell grid and the brute-force scan give the same (j, d2) bits, for
 * every cell edge.
 *
 * Start.  T = guess (double 4x4, row-major, rigid); p_i = (float)(((r00*x + r01*y) + r02*z) + t0) and so on, in double
 * from the float source point.
 *
 * Iteration k = 1, 2, ...  Correspondences of the current p_i: n of them.  n < min_correspondences: stop, not converged,
 * DLIOM_ICP_NO_CORRESPONDENCES, T and p_i stay, `iterations` = k - 1.  Else sixteen sums in double from the float values
 * of p_i and q_i = t_j(i): Sp (3), Sq (3), Spq[a][b] = sum p_a * q_b (9, the RAW moments, one pass; the products are
 * exact in double) and Sd = sum (double)d2.  Every sum runs over the SOURCE INDEX with +0.0 where there is no
 * correspondence, in one fixed tree: pad to max(2048, the next power of two) leaves with +0.0, then add adjacent pairs
 * level by level -- a function of the index alone.  (Leaves beyond the next power of two change nothing but a root of
 * -0.0.)
 * Solve: cp = Sp / n, cq = Sq / n, H[a][b] = Spq[a][b] - (Sp[a] * Sq[b]) / n.  Horn's matrix
 *     N = [ Hxx+Hyy+Hzz  Hyz-Hzy      Hzx-Hxz      Hxy-Hyx
 *           .            Hxx-Hyy-Hzz  Hxy+Hyx      Hzx+Hxz
 *           .            .            (Hyy-Hxx)-Hzz  Hyz+Hzy
 *           .            .            .            (Hzz-Hxx)-Hyy ]  (symmetric),
 * its eigenvectors by DLIOM_ICP_JACOBI_SWEEPS cyclic Jacobi sweeps over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), each
 * rotation (skipped when a_pq == 0): theta = (a_qq - a_pp) / (2 * a_pq); tt = (theta >= 0 ? 1 : -1) / (|theta| +
 * sqrt(theta * theta + 1)); c = 1 / sqrt(tt * tt + 1); s = tt * c; a_pp -= tt * a_pq; a_qq += tt * a_pq; a_pq = 0; for
 * r != p, q: (a_rp, a_rq) = (c * a_rp - s * a_rq, s * a_rp + c * a_rq); for every r: (v_rp, v_rq) likewise.  The
 * quaternion (w, x, y, z) is the column of V with the greatest diagonal entry (ties to the lowest column), divided by
 * its norm sqrt(((w*w + x*x) + y*y) + z*z); R is its rotation matrix, R00 = 1 - 2 * (y*y + z*z), R01 = 2 * (x*y - z*w),
 * R02 = 2 * (x*z + y*w), R10 = 2 * (x*y + z*w), R11 = 1 - 2 * (x*x + z*z), R12 = 2 * (y*z - x*w), R20 = 2 * (x*z - y*w),
 * R21 = 2 * (y*z + x*w), R22 = 1 - 2 * (x*x + y*y); t_a = cq_a - ((R_a0 * cp_0 + R_a1 * cp_1) + R_a2 * cp_2).  Only IEEE
 * double + - * / sqrt, a fixed count, on the host.  A degenerate H (collinear pairs: the greatest eigenvalue repeated)
 * has no rule of its own: the procedure's output is a proper rotation that attains the least squares, one of several.
 * Then p_i <- (float)(R p_i + t) in the order of Start, T <- M T with M = [R t; 0 0 0 1] (each entry ((m0*t0 + m1*t1) +
 * m2*t2), the translation column + m3), mse_k = Sd / n.
 *
 * Convergence, tested in this order after iteration k (mse_0 = +inf):
 *   1. k >= maximum_iterations: DLIOM_ICP_ITERATIONS, reported as converged like PCL does (so 0 runs one iteration);
 *   2. 0.5 * (((R00 + R11) + R22) - 1) >= 1 - rotation_epsilon and (tx*tx + ty*ty) + tz*tz <= transformation_epsilon:
 *      DLIOM_ICP_TRANSFORM;
 *   3. |mse_k - mse_{k-1}| < euclidean_fitness_epsilon: DLIOM_ICP_ABS_MSE;
 *   4. |mse_k - mse_{k-1}| / mse_{k-1} < relative_mse_epsilon: DLIOM_ICP_REL_MSE.
 * After the first iteration 3 compares +inf and 4 compares inf / inf = NaN: both false, as is 0 / 0 in 4.
 *
 * Fitness score (getFitnessScore()): one more search on the final p_i without a distance bound; the mean of d2 over
 * the source points that have a neighbour, by the same tree; the count is reported.
 *
 * No floating-point atomics anywhere: two calls on one input give the same bytes.  Malformed input fails with
 * DLIOM_ERR_INVALID_ARGUMENT before anything runs: NULLs, a non-finite or negative option (the correspondence distance
 * alone may be +inf), maximum_iterations < 0, min_correspondences < 3, a guess with a non-finite entry, a last row other
 * than 0 0 0 1 or |R^T R - I| > 1e-6 in any entry or det R <= 0, clouds of another context, and an EMPTY target cloud.
 * A target whose points are all non-finite is accepted: no query has a neighbour, an alignment ends with
 * DLIOM_ICP_NO_CORRESPONDENCES. */
#define DLIOM_NN_MAX_SHELLS 3        /* shells of cells walked around a query's cell before the brute-force scan takes it */
#define DLIOM_NN_MAX_CELLS_PER_AXIS 1024
#define DLIOM_NN_MAX_CELLS (1 << 22)
#define DLIOM_NN_MAX_POINTS (1 << 24) /* of a target and of a query cloud */
#define DLIOM_ICP_JACOBI_SWEEPS 12
#define DLIOM_ICP_TREE_MIN_LEAVES 2048
enum { DLIOM_NN_AUTO = 0, DLIOM_NN_BRUTE_FORCE = 1 };
enum {
  DLIOM_ICP_NOT_CONVERGED = 0,
  DLIOM_ICP_ITERATIONS = 1,
  DLIOM_ICP_TRANSFORM = 2,
  DLIOM_ICP_ABS_MSE = 3,
  DLIOM_ICP_REL_MSE = 4,
  DLIOM_ICP_NO_CORRESPONDENCES = 5
};
typedef struct dliom_nn_index dliom_nn_index;
typedef struct dliom_nn_index_options {
  double cell_edge; /* metres; 0: automatic (half the edge that puts one point a cell into the bounding box).  Grown until
                       the grid fits DLIOM_NN_MAX_CELLS_PER_AXIS and DLIOM_NN_MAX_CELLS.  Results never depend on it. */
  int search;       /* DLIOM_NN_*: what DLIOM_NN_AUTO means for this index's queries */
  int reserved;     /* 0 */
} dliom_nn_index_options;
typedef struct dliom_nn_query_stats {
  int64_t queries, non_finite;       /* non_finite: queries without a search */
  int64_t settled_by_grid;           /* by the shell walk */
  int64_t settled_by_brute_force;    /* by the brute-force scan */
  int64_t read_backs;
  double search_ms;                  /* filled only while the context's profiling is on */
} dliom_nn_query_stats;
typedef struct dliom_nn_index_memory {
  int64_t points, finite_points, cells, dims[3], index_bytes, scratch_bytes;
  double cell_edge; /* the edge in use */
} dliom_nn_index_memory;
typedef struct dliom_icp_options {
  double max_correspondence_distance;
  double transformation_epsilon;     /* on the squared translation */
  double euclidean_fitness_epsilon;
  double rotation_epsilon;           /* 1 - PCL's cosine 0.99999 */
  double relative_mse_epsilon;
  int maximum_iterations;
  int min_correspondences;
  int search;                        /* DLIOM_NN_* */
  int reserved;                      /* 0 */
} dliom_icp_options;
typedef struct dliom_icp_result {
  int converged, reason, iterations; /* reason: DLIOM_ICP_* */
  int correspondences;               /* of the last search of the loop */
  double transform[16];              /* T, row-major */
  double mse;                        /* of the last completed iteration; +inf if there is none */
  double fitness_score;              /* NaN when fitness_count is 0 */
  int64_t fitness_count;
  int64_t read_backs;                /* polled read-backs of the call: one an iteration's sums, one for the fitness score */
  int64_t settled_by_grid, settled_by_brute_force; /* over every search of the call */
  /* milliseconds of the stages over all iterations (solve_ms: host time of solve and decision); filled (the call then
   * synchronises the stream) only while the context's profiling is on */
  double search_ms, reduce_ms, solve_ms, transform_ms;
} dliom_icp_result;
/* Builds the cell grid over the finite points of `target` (one polled read-back: the bounding box).  The index keeps its
 * own copy of the points: the cloud may be destroyed.  One thread at a time per index, like its context; destroy the
 * index before the context.  options may be NULL (automatic edge, DLIOM_NN_AUTO). */
int dliom_nn_index_create(dliom_ctx* ctx, const dliom_cloud* target, const dliom_nn_index_options* options,
                          dliom_nn_index** index);
void dliom_nn_index_destroy(dliom_nn_index* index);
int dliom_nn_index_memory_stats(const dliom_nn_index* index, dliom_nn_index_memory* out);
/* The neighbour of every point of `queries` (transformed by transform16 as in Start when it is not NULL) within
 * max_distance (+inf: no bound): j_out[i] = -1 and d2_out[i] = +inf where there is none.  search: DLIOM_NN_AUTO (the
 * index's own choice) or DLIOM_NN_BRUTE_FORCE.  stats may be NULL. */
int dliom_nn_index_query(dliom_nn_index* index, const dliom_cloud* queries, const double* transform16, double max_distance,
                         int search, int32_t* j_out, float* d2_out, dliom_nn_query_stats* stats);

/* Many indices in one call: the tool's other per-target build (gen_ground_truth_by_ndt_match.cc:199-200, setInputTarget of
 * every distinct ICP target, and :219, the index behind an NDT pair's getFitnessScore()).  The clouds of a chunk go through
 * ONE launch chain, whatever their number, with the cloud's slot as a grid dimension: the bounding boxes, one read-back,
 * and the counting sort by cell with ONE scan over the concatenation of many indices' cell arrays.  Every kernel runs the
 * body that dliom_nn_index_create's kernel runs, on the cloud's own points with the cloud's own grid.
 *
 * Results.  out[i] is a dliom_nn_index like any other: destroyed on its own with dliom_nn_index_destroy, in any order and
 * before or after its cloud, and usable with dliom_nn_index_query, dliom_icp_align, dliom_icp_step, dliom_icp_align_batch
 * and as a fitness_index of dliom_ndt_align and dliom_ndt_align_batch.  dliom_nn_index_memory_stats gives the single build's
 * points, finite_points, cells, dims, cell_edge and index_bytes (not scratch_bytes: a batch-built index has no scratch
 * until its first call).  Every query gives, bit for bit, what it gives on the index that dliom_nn_index_create(ctx,
 * clouds[i], options, ...) builds: j, d2, settled_by_grid, settled_by_brute_force and non_finite.  The order of the points
 * inside a cell is unspecified, as the single build's is; no result depends on it.  A cloud may be named more than once;
 * each mention gets an index of its own.  Results never depend on the limits, on the order of the clouds, or on which
 * other clouds share a chunk.
 *
 * Schedule.  Chunks are consecutive runs of clouds in input order.  A chunk closes when it holds max_indices_in_flight
 * clouds, or when adding the next cloud would take the chunk's point sum above max_points_in_flight; it always holds at
 * least one cloud.  A chunk costs one upload of its clouds' descriptors, one launch of the bounding boxes and ONE polled
 * read-back: eight words a cloud, the ordered box words and the finite count.  The host then chooses every grid as the
 * single build does, makes ONE device allocation an index (by_index | cell_start | sorted: all three sizes are known by
 * then) and uploads the descriptors again, with the grids and the arrays.  The chunk's indices then go through the
 * counting sort in CELL RUNS: consecutive indices whose cells + 1 sum to at most max_cells_in_flight, at least one index a
 * run (an index has at most DLIOM_NN_MAX_CELLS cells, so a run's positions fit an int).  A cell run is one memset, one
 * launch that counts, ONE exclusive sum over the concatenation of the run's cell arrays, and one launch that scatters and
 * writes each index's own cell_start, the scan's value minus its value at the index's first cell.  Runs add launches,
 * never read-backs.  (A launch holds at most 2^30 lanes; a chunk of very many very long clouds splits its launches by
 * slots.)  ONE stream synchronisation ends a chunk: after it the descriptor table is free for the next chunk and the
 * clouds are the caller's again.  read_backs == synchronizations == chunks, and cell_runs is the sum over the chunks.  The
 * work space is one growable block on the context, kept until the context is destroyed: the descriptors and the box words
 * before the read-back; the descriptors, a cell a point (4 bytes) and the populations, cursors and scan of the largest
 * cell run after it, sized exactly (scratch_bytes: the larger of the two over the chunks).
 *
 * Refusals, all before anything runs (DLIOM_ERR_INVALID_ARGUMENT, no read-back or synchronisation counted on the context):
 * a NULL context or out; NULL clouds with count > 0; count < 0; options that dliom_nn_index_create refuses (NULL: the
 * defaults, one set for all); limits outside their ranges or reserved != 0; a NULL cloud, a cloud of another context, an
 * empty cloud, a cloud above DLIOM_NN_MAX_POINTS.  count == 0 succeeds and launches nothing.  A HIP or allocation failure
 * fails the whole call, destroys what was built and leaves every out[i] NULL.  There is no per-index status. */
#define DLIOM_NN_INDEX_BATCH_MAX_INDICES 256
typedef struct dliom_nn_index_batch_limits {
  int max_indices_in_flight;      /* 1 .. DLIOM_NN_INDEX_BATCH_MAX_INDICES; default 64 */
  int reserved;                   /* 0 */
  int64_t max_points_in_flight;   /* 1 .. 2^30; default 64 * DLIOM_NDT_BATCH_DEFAULT_POINTS */
  int64_t max_cells_in_flight;    /* 1 .. 2^30; default 2^26 */
} dliom_nn_index_batch_limits;    /* NULL = the defaults, which dliom_nn_index_batch_default_limits() returns */
typedef struct dliom_nn_index_batch_stats {
  int64_t indices, chunks, cell_runs;
  int64_t points, finite_points, cells;   /* summed over the indices */
  int64_t read_backs;             /* polled read-backs of the call: one a chunk */
  int64_t synchronizations;       /* stream synchronisations of the call: one a chunk */
  int64_t max_in_flight;          /* the largest chunk, in indices */
  int64_t scratch_bytes;          /* the largest chunk's device work space */
  double box_ms, sort_ms, alloc_ms; /* descriptors, boxes and the read-back | the second upload, the cell runs and the
                                     synchronisation | the grids' choice and the allocations; on the host's clock, only
                                     while the context's profiling is on */
} dliom_nn_index_batch_stats;
int dliom_nn_index_batch_default_limits(dliom_nn_index_batch_limits* limits);
int dliom_nn_index_create_batch(dliom_ctx* ctx, const dliom_cloud* const* clouds, int count,
                                const dliom_nn_index_options* options /* may be NULL, one for all */,
                                const dliom_nn_index_batch_limits* limits, dliom_nn_index** out /* count entries */,
                                dliom_nn_index_batch_stats* stats /* may be NULL */);

/* The tool's values (gen_ground_truth_by_ndt_match.cc:192-196): 30 m, 100 iterations, both epsilons 1e-6. */
int dliom_icp_default_options(dliom_icp_options* options);
/* Aligns `source` to the index's target from guess16.  aligned (may be NULL): the final p_i as a cloud of the context. */
int dliom_icp_align(dliom_nn_index* index, const dliom_cloud* source, const double* guess16, const dliom_icp_options* options,
                    dliom_icp_result* result, dliom_cloud** aligned);
/* Diagnostic: one iteration from the given points (no guess): their correspondences (j, d2 as dliom_nn_index_query
 * gives them), the sixteen sums (Sp, Sq, Spq row-major, Sd), n, and R (row-major), t -- the identity when
 * n < min_correspondences. */
int dliom_icp_step(dliom_nn_index* index, const dliom_cloud* points, const dliom_icp_options* options, int32_t* j_out,
                   float* d2_out, double* sums16, int64_t* correspondences, double* rotation9, double* translation3);

/* Many pairs in one call: gen_ground_truth_by_ndt_match.cc:151-261 aligns the two scans of EVERY inter-submap constraint of
 * a trajectory, hundreds to thousands of independent alignments.  All pairs of a chunk advance in lock step: a step is one
 * search of every pair still in flight, in ONE launch chain with ONE polled read-back, whatever the number of pairs.
 *
 * Results.  results[i] is what dliom_icp_align(pairs[i].index, pairs[i].source, pairs[i].guess, options, ...) returns, bit
 * for bit, in converged, reason, iterations, correspondences, transform, mse, fitness_score, fitness_count, read_backs (the
 * searches the pair took part in), settled_by_grid and settled_by_brute_force (from a counter block of the pair's own,
 * zeroed at its start).  The four *_ms fields of a result are 0; the stages' times are in the statistics.  aligned[i] is the
 * single call's cloud, norm bound included.  Results never depend on the limits or on the order of the pairs.
 *
 * Schedule.  Chunks are consecutive runs of pairs in input order.  A chunk closes when it holds max_pairs_in_flight pairs,
 * or when adding the next pair's dliom_icp_batch_scratch_bytes(n) would take the chunk's sum above max_scratch_bytes; it
 * always holds at least one pair.  Chunks are not refilled: a chunk takes as many steps as the pair of it with the most
 * searches, `steps` is the sum over the chunks, and read_backs == steps.
 *
 * Refusals, all before anything runs (DLIOM_ERR_INVALID_ARGUMENT): a NULL context or options; NULL pairs or results
 * with count > 0; count < 0; options that dliom_icp_align refuses; limits outside their ranges; a pair with a NULL index
 * or source, with an index or a cloud of another context, or with a guess that dliom_icp_align refuses.  count == 0
 * succeeds and launches nothing.  A HIP or allocation failure fails the whole call and leaves no cloud behind (every
 * aligned[i] is NULL).  There is no per-pair status: the single call has no refusal of a pair that passes these checks. */
#define DLIOM_ICP_BATCH_MAX_PAIRS 256
typedef struct dliom_icp_pair {
  dliom_nn_index* index;        /* the target; any number of pairs may name one index */
  const dliom_cloud* source;    /* any number of pairs may name one cloud */
  double guess[16];             /* as dliom_icp_align's guess16 */
} dliom_icp_pair;
typedef struct dliom_icp_batch_limits {
  int max_pairs_in_flight;      /* 1 .. DLIOM_ICP_BATCH_MAX_PAIRS; default 64 */
  int reserved;                 /* 0 */
  int64_t max_scratch_bytes;    /* > 0; default 1 GiB */
} dliom_icp_batch_limits;       /* NULL = the defaults, which dliom_icp_batch_default_limits() returns */
typedef struct dliom_icp_batch_stats {
  int64_t pairs, chunks, steps; /* steps: lock-step rounds (one search of every pair still in flight) */
  int64_t read_backs;           /* polled read-backs of the call == steps */
  int64_t synchronizations;     /* stream synchronisations of the call: one a chunk when `aligned` is given (its clouds are
                                   copied out of the chunk's scratch), one for the stages' times while profiling is on */
  int64_t pair_searches;        /* sum over pairs of the searches they took part in == sum of results[i].read_backs */
  int64_t max_in_flight;        /* the largest chunk */
  double search_ms, reduce_ms, solve_ms, transform_ms;  /* only while the context's profiling is on */
} dliom_icp_batch_stats;
int dliom_icp_batch_default_limits(dliom_icp_batch_limits* limits);
/* Host only: the device scratch that one pair in flight with source_points points reserves (0 for a negative count). */
int64_t dliom_icp_batch_scratch_bytes(int64_t source_points);
int dliom_icp_align_batch(dliom_ctx* ctx, const dliom_icp_pair* pairs, int count, const dliom_icp_options* options,
                          const dliom_icp_batch_limits* limits, dliom_icp_result* results,
                          dliom_cloud** aligned /* NULL, or count entries */, dliom_icp_batch_stats* stats /* may be NULL */);

/* ---- scan alignment by NDT ------------------------------------------------------------------------------
 * pcl::NormalDistributionsTransform as the reference runs it: LocalTrajectoryBuilder3D::MatchByNDT
 * (local_trajectory_builder_3d.cc:969-1008: epsilon 0.01, step 0.1, resolution 1.0, 35 iterations, on clouds filtered by
 * pcl::ApproximateVoxelGrid at 0.2 m) and gen_ground_truth_by_ndt_match.cc's `--method ndt` (:211-222, the same four
 * values, on raw scans).  PARITY UNPINNED AGAINST PCL, for the reason given in the ICP section.  What is pinned, bit for bit
 * against a CPU model (tests/ndt_common.py), is this definition, our reading of PCL 1.8.0's VoxelGridCovariance and
 * NormalDistributionsTransform; where it differs from PCL, this text governs.  Arithmetic is double unless said otherwise,
 * every operation rounded on its own, in the order written, parentheses first and otherwise left to right.  min(a, b) is
 * (b < a ? b : a) and max(a, b) is (a < b ? b : a).
 *
 * TARGET CELLS.  inv = 1.0f / (float)resolution.  The cell of a target point is (floor(x*inv), floor(y*inv), floor(z*inv))
 * in float.  A point with a non-finite coordinate, or with a cell index outside [-2^20, 2^20) on any axis, is skipped.
 * Cells are kept sparsely (sorted 63-bit keys, z high, x low): there is no dense box.  For each cell n, S_a = sum x_a (3) and
 * Q_ab = sum x_a * x_b for a <= b (6; float * float is exact in double), each over the cell's points in ascending point
 * index in one fixed tree: pad to the next power of two with +0.0, then add adjacent pairs level by level.
 * Per cell, on the host: mean_a = S_a / n; for a <= b, mirrored,
 *     C_ab = ((Q_ab - 2 * (S_a * mean_b)) / n + mean_a * mean_b) * ((n - 1.0) / n).
 * Eigen-decomposition of C by DLIOM_NDT_JACOBI_SWEEPS cyclic Jacobi sweeps over (0,1) (0,2) (1,2) with ICP's rotation
 * rule; eigenvalues l0 <= l1 <= l2 by a stable sort of the diagonal (ties keep column order), v_k the matching columns.
 * The cell is VALID iff n >= min_points_per_voxel, l0 >= 0, l1 >= 0, l2 > 0 and every entry of icov is finite, where
 * l0 and l1 are first raised to 0.01 * l2 if below it and, for a <= b, mirrored,
 *     icov_ab = ((v_a0*v_b0)/l0 + (v_a1*v_b1)/l1) + (v_a2*v_b2)/l2.
 * (The test on n comes first: a cell with n < min_points_per_voxel has no C.)  An invalid cell is never a neighbour; PCL
 * leaves such a leaf in its kd-tree with stale values.
 *
 * NEIGHBOURS of a query q (float xyz).  q without a finite coordinate, or whose cell index lies outside [-2^20 - 1, 2^20]
 * on an axis, has none.  Candidates: the valid cells whose index differs from q's by at most 1 on every axis, visited z
 * outermost, x fastest, each from -1.  A candidate is a neighbour iff, in float with m = (float)mean, dx = q.x - m.x and so
 * on, (dx*dx + dy*dy) + dz*dz <= r2, r2 = (float)resolution * (float)resolution, inclusive.  This stands for PCL's FLANN
 * radius search over the centroids.
 *
 * CONSTANTS (host libm log and exp), o = outlier_ratio: c1 = 10 * (1 - o); c2 = o / ((resolution * resolution) *
 * resolution); d3 = -log(c2); d1 = -log(c1 + c2) - d3; d2 = -2 * log((-log(c1 * exp(-0.5) + c2) - d3) / d1).
 *
 * POSE.  p = (tx, ty, tz, a, b, c), T(p) = [R t], R = Rx(a) Ry(b) Rz(c); sa, ca, sb, cb, sc, cc from host libm (no
 * small-angle shortcut).  A product of three factors is (u*v)*w.  Rows of R:
 *     (cb*cc, -cb*sc, sb)   (ca*sc + sa*sb*cc, ca*cc - sa*sb*sc, -sa*cb)   (sa*sc - ca*sb*cc, sa*cc + ca*sb*sc, ca*cb).
 * From a guess (checked as ICP checks it): t = its last column, a = atan2(-R12, R22), b = atan2(R02, sqrt(R00*R00 +
 * R01*R01)), c = atan2(-R01, R00): Eigen's eulerAngles(0,1,2) rotation, not its branch.  A transformed point is
 * x' = (float)(((r0*x + r1*y) + r2*z) + t) row by row, as in ICP's Start; x below is the (double) source point itself.
 *
 * POINT DERIVATIVES.  J_0..2 are the unit vectors; J_3 = d(Rx)/da, J_4 = d(Rx)/db, J_5 = d(Rx)/dc; H_ij = d2(Rx)/dp_i dp_j
 * (zero unless i, j >= 3).  Each component is a row of coefficients k dotted with x as (k0*x0 + k1*x1) + k2*x2; a
 * component not listed is +0.0.  The rows (Magnusson 2009, eq. 6.19 and 6.21):
 *   J_3: [1] (-sa*sc + ca*sb*cc, -sa*cc - ca*sb*sc, -ca*cb)   [2] (ca*sc + sa*sb*cc, ca*cc - sa*sb*sc, -sa*cb)
 *   J_4: [0] (-sb*cc, sb*sc, cb)   [1] (sa*cb*cc, -sa*cb*sc, sa*sb)   [2] (-ca*cb*cc, ca*cb*sc, -ca*sb)
 *   J_5: [0] (-cb*sc, -cb*cc, 0)   [1] (ca*cc - sa*sb*sc, -ca*sc - sa*sb*cc, 0)   [2] (sa*cc + ca*sb*sc, -sa*sc + ca*sb*cc, 0)
 *   H_33: [1] (-ca*sc - sa*sb*cc, -ca*cc + sa*sb*sc, sa*cb)   [2] (-sa*sc + ca*sb*cc, -sa*cc - ca*sb*sc, -ca*cb)
 *   H_34: [1] (ca*cb*cc, -ca*cb*sc, ca*sb)   [2] (sa*cb*cc, -sa*cb*sc, sa*sb)
 *   H_35: [1] (-sa*cc - ca*sb*sc, sa*sc - ca*sb*cc, 0)   [2] (ca*cc - sa*sb*sc, -ca*sc - sa*sb*cc, 0)
 *   H_44: [0] (-cb*cc, cb*sc, -sb)   [1] (-sa*sb*cc, sa*sb*sc, sa*cb)   [2] (ca*sb*cc, -ca*sb*sc, -ca*cb)
 *   H_45: [0] (sb*sc, sb*cc, 0)   [1] (-sa*cb*sc, -sa*cb*cc, 0)   [2] (ca*cb*sc, ca*cb*cc, 0)
 *   H_55: [0] (-cb*cc, cb*sc, 0)   [1] (-ca*sc - sa*sb*cc, -ca*cc + sa*sb*sc, 0)   [2] (-sa*sc + ca*sb*cc, -sa*cc - ca*sb*sc, 0)
 * Negation is exact, so a signed two-term entry has one value whatever the order of its terms.  The host computes the
 * 8 + 15 rows once an evaluation.
 *
 * EVALUATION at p.  For every source point i and every neighbour cell of x'_i in the order above, xt = (double)x' - mean:
 *   w_r = (icov_r0*xt0 + icov_r1*xt1) + icov_r2*xt2;  q = (xt0*w0 + xt1*w1) + xt2*w2;  e = E(-(d2 * q) * 0.5);
 *   f = d2 * e;  if f > 1, f < 0 or f is NaN the cell adds nothing (it is still counted as a pair).  Otherwise
 *   score += -d1 * e;  f = f * d1;  with cJ_i = icov J_i (rows as w; for i < 3 this is column i of icov) and
 *   u_i = (xt0*cJ_i0 + xt1*cJ_i1) + xt2*cJ_i2:
 *   g_i += u_i * f;
 *   H_ij += f * ((((-d2) * u_i) * u_j + h_ij) + k_ij) for i <= j, mirrored, where h_ij = xt . (icov H_ij) (rows as w, dot as
 *   q; +0.0 unless i, j >= 3) and k_ij = (J_j0*cJ_i0 + J_j1*cJ_i1) + J_j2*cJ_i2 (for j < 3 this is cJ_ij).
 * A point's 28 values (score, g 0..5, H 00 01 .. 05 11 12 .. 55) start at +0.0 and are summed over its cells in that order;
 * the 28 sums over the source index run in ICP's fixed tree (DLIOM_ICP_TREE_MIN_LEAVES), with +0.0 for a point without
 * neighbours.  The count of (point, neighbour cell) pairs is reported.  An evaluation may leave out the Hessian, or
 * compute the Hessian alone; what it computes has the same bits.
 * E(u): +0.0 for u < -708; u itself for a NaN; +inf for u > 708; otherwise k = the nearest integer to
 * u * 0x1.71547652b82fep+0 (ties to even), r = (u - k * 0x1.62e42fee00000p-1) - k * 0x1.a39ef35793c76p-33, Horner's rule
 * p = p * r + c_n from p = c_13 down to c_0, c_n = 1/n! rounded to double, and the result is p * 2^k (exact).  Within
 * 1.14 ulp of the correctly rounded exponential on [-708, 0] (measured on a CPU, 800 000 arguments).
 *
 * ALIGNMENT.  Evaluate at the guess's p (with the Hessian).  Then, from it = 0:
 *   1. delta = -pinv(H) g: DLIOM_NDT_PINV_SWEEPS cyclic Jacobi sweeps on the symmetric 6x6 (pairs (0,1) (0,2) .. (4,5), ICP's
 *      rule) give l_k and V; y_k = sum_r V_rk * g_r; z_k = y_k / l_k if |l_k| > 6 * 2^-52 * max|l|, else +0.0;
 *      delta_r = -(sum_k V_rk * z_k); the sums left to right from +0.0.  It stands for PCL's JacobiSVD solve.
 *   2. s = sqrt of the sum of delta_r^2 (left to right).  s == 0 or NaN: stop, DLIOM_NDT_ZERO_STEP, converged iff s == s;
 *      `iterations` = it.
 *   3. dir = delta / s; a = step_length (below); p_r <- p_r + dir_r * a (the point of the step's last evaluation).
 *   4. Stop, converged, iff it > maximum_iterations (DLIOM_NDT_ITERATIONS) or (it > 0 and |a| < transformation_epsilon)
 *      (DLIOM_NDT_EPSILON); `iterations` = it + 1.
 *   5. it += 1.
 * transformation_probability = score / N, N = every source point; score, g, H are those of the last evaluation.
 *
 * STEP LENGTH (computeStepLengthMT), step_max = step_size, step_min = transformation_epsilon / 2.
 *   phi0 = -score; dphi0 = -(g . dir) (left to right).  dphi0 == 0: return 0 (nothing is evaluated).  dphi0 > 0: negate
 *   dphi0 and dir (the caller's too).  a_t = max(min(s, step_max), step_min).  Evaluate at p + dir*a_t with the Hessian.
 *   DLIOM_NDT_STEP_CLAMPED: return a_t.  This is PCL 1.8.0, whose interval test `(step_max - step_min) > 0` makes the
 *   search loop unreachable.
 *   DLIOM_NDT_STEP_MORE_THUENTE (as later PCL): mu = 1e-4, nu = 0.9; a_l = a_u = 0; f_l = f_u = 0 (psi(0));
 *   g_l = g_u = dphi0 - mu * dphi0; open = true; phi_t = -score, dphi_t = -(g . dir), psi_t = (phi_t - phi0) - (mu * dphi0) * a_t,
 *   dpsi_t = dphi_t - mu * dphi0.  While fewer than 10 trials ran, the interval has not converged and not (psi_t <= 0 and
 *   dphi_t <= -nu * dphi0): a_t = trial(..., psi_t, dpsi_t) if open else trial(..., phi_t, dphi_t); a_t = max(min(a_t,
 *   step_max), step_min); evaluate at p + dir*a_t WITHOUT the Hessian; phi_t, dphi_t, psi_t, dpsi_t anew; if open and
 *   psi_t <= 0 and dpsi_t >= 0: open = false, f_l = (f_l + phi0) - (mu * dphi0) * a_l, g_l = g_l + mu * dphi0, likewise u;
 *   then the interval update with (psi_t, dpsi_t) if open, else (phi_t, dphi_t).  If any trial ran, one Hessian-only
 *   evaluation at the final point.
 *   trial(a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t): z = (3 * (f_t - f_l) / (a_t - a_l) - g_t) - g_l; w = sqrt(z*z - g_t*g_l);
 *   a_c = a_l + (a_t - a_l) * ((w - g_l) - z) / ((g_t - g_l) + 2 * w).
 *     1. f_t > f_l: a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t)); a_c if |a_c - a_l| < |a_q - a_l|,
 *        else 0.5 * (a_q + a_c).
 *     2. else g_t * g_l < 0: a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l; a_c if |a_c - a_t| >= |a_s - a_t|, else a_s.
 *     3. else |g_t| <= |g_l|: a_s as in 2; n = a_c if |a_c - a_t| < |a_s - a_t| else a_s; min(a_t + 0.66 * (a_u - a_t), n) if
 *        a_t > a_l, else the max of the two.
 *     4. else: z = (3 * (f_t - f_u) / (a_t - a_u) - g_t) - g_u; w = sqrt(z*z - g_t*g_u);
 *        a_u + (a_t - a_u) * ((w - g_u) - z) / ((g_t - g_u) + 2 * w).
 *   Interval update: 1. f_t > f_l: u <- t.  2. else g_t * (a_l - a_t) > 0: l <- t.  3. else g_t * (a_l - a_t) < 0: u <- l, then
 *   l <- t.  4. else: converged.
 *
 * FITNESS SCORE (the tool's getFitnessScore()): with a dliom_nn_index of the target, ICP's: one search on the final
 * x'_i without a bound, the mean of d2 by the same tree; NaN and count 0 without an index.
 *
 * No floating-point atomics anywhere: two calls on one input give the same bytes.  Malformed input fails with
 * DLIOM_ERR_INVALID_ARGUMENT before anything runs: NULLs, clouds (or an index) of another context, a non-finite or
 * non-positive resolution or step size, an outlier ratio outside (0, 1), a negative or non-finite epsilon, a negative
 * maximum_iterations, min_points_per_voxel < 3, an unknown step mode, options whose resolution is not the target's, a bad
 * guess, an empty target.  A target without a valid cell is accepted: every evaluation is all zeros and the alignment ends
 * with DLIOM_NDT_ZERO_STEP. */
#define DLIOM_NDT_JACOBI_SWEEPS 8    /* 3x3, per cell */
#define DLIOM_NDT_PINV_SWEEPS 12     /* 6x6, per iteration */
#define DLIOM_NDT_MAX_CELL_INDEX (1 << 20)
enum { DLIOM_NDT_STEP_CLAMPED = 0, DLIOM_NDT_STEP_MORE_THUENTE = 1 };
enum { DLIOM_NDT_NOT_CONVERGED = 0, DLIOM_NDT_ITERATIONS = 1, DLIOM_NDT_EPSILON = 2, DLIOM_NDT_ZERO_STEP = 3 };
enum { DLIOM_NDT_EVAL_GRADIENT = 0, DLIOM_NDT_EVAL_ALL = 1, DLIOM_NDT_EVAL_HESSIAN = 2 };
typedef struct dliom_ndt_target dliom_ndt_target;
typedef struct dliom_ndt_options {
  double resolution;             /* metres a cell */
  double step_size;              /* step_max */
  double transformation_epsilon;
  double outlier_ratio;
  int maximum_iterations;
  int min_points_per_voxel;
  int step_mode;                 /* DLIOM_NDT_STEP_* */
  int reserved;                  /* 0 */
} dliom_ndt_options;
typedef struct dliom_ndt_cell {
  int32_t index[3];
  int32_t valid;
  int64_t n;
  double mean[3];
  double icov[6];                /* 00 01 02 11 12 22; zeros for an invalid cell */
} dliom_ndt_cell;
typedef struct dliom_ndt_target_memory {
  int64_t points, kept_points, cells, valid_cells, target_bytes, scratch_bytes;
  int64_t read_backs;            /* of the build */
  double build_ms;               /* keys, sort, sums, the host step and the upload; filled only under profiling */
} dliom_ndt_target_memory;
typedef struct dliom_ndt_result {
  int converged, reason, iterations; /* reason: DLIOM_NDT_* */
  int reserved;
  int64_t evaluations_with_hessian, evaluations_without_hessian; /* a Hessian-only evaluation counts as with */
  double p[6];
  double transform[16];              /* T(p), row-major */
  double score, transformation_probability;
  double fitness_score;              /* NaN when fitness_count is 0 */
  int64_t fitness_count;
  int64_t pairs;                     /* (point, neighbour cell) pairs of the last evaluation */
  int64_t read_backs;                /* one an evaluation, one for the fitness score */
  /* milliseconds over all evaluations (host_ms: pseudo-inverse, step length and decisions); filled (the call then
   * synchronises the stream) only while the context's profiling is on */
  double evaluate_ms, reduce_ms, host_ms;
} dliom_ndt_result;
/* The tool's and the front end's values: resolution 1.0, step 0.1, epsilon 0.01, 35 iterations; PCL's 0.55 and 6;
 * DLIOM_NDT_STEP_CLAMPED. */
int dliom_ndt_default_options(dliom_ndt_options* options);
/* Builds the cells of `target` (resolution and min_points_per_voxel of `options`): two round trips (the cell count, then
 * the sums) and one upload.  The cloud may be destroyed afterwards.  One thread at a time per target, like its context;
 * destroy the target before the context. */
int dliom_ndt_target_create(dliom_ctx* ctx, const dliom_cloud* target, const dliom_ndt_options* options, dliom_ndt_target** out);
void dliom_ndt_target_destroy(dliom_ndt_target* target);
int dliom_ndt_target_memory_stats(const dliom_ndt_target* target, dliom_ndt_target_memory* out);
/* Diagnostic: every cell in key order (z, then y, then x).  cells == NULL: only *count.  capacity < *count: DLIOM_ERR_CAPACITY. */
int dliom_ndt_target_cells(const dliom_ndt_target* target, dliom_ndt_cell* cells, int64_t capacity, int64_t* count);
/* Diagnostic: one evaluation at p6.  what: DLIOM_NDT_EVAL_*; what is not computed comes back as zeros.  hessian36 is
 * row-major and mirrored. */
int dliom_ndt_evaluate(dliom_ndt_target* target, const dliom_cloud* source, const double* p6, const dliom_ndt_options* options,
                       int what, double* score, double* gradient6, double* hessian36, int64_t* pairs);
/* Aligns `source` to the target from guess16.  fitness_index (may be NULL): an index of the target's cloud on the same
 * context.  aligned (may be NULL): the final x'_i as a cloud of the context. */
int dliom_ndt_align(dliom_ndt_target* target, const dliom_cloud* source, const double* guess16, const dliom_ndt_options* options,
                    dliom_nn_index* fitness_index, dliom_ndt_result* result, dliom_cloud** aligned);
/* LocalTrajectoryBuilder3D::MatchByNDT (local_trajectory_builder_3d.cc:969-1008) as InitilizeByNDT (:231-330, the
 * reference's spelling) calls it: every scan is aligned to its predecessor, so the matcher keeps the previous scan's cells
 * on the device.  The first match only filters the scan (the approximate voxel grid above, at `leaf`: the reference's
 * 0.2 m), builds its cells and keeps them; guess16 and result may be NULL and nothing is written to result.  Every later
 * match filters the new scan ONCE, aligns it to the kept cells from guess16 as dliom_ndt_align does without a fitness
 * index, builds the new scan's cells and makes them the kept ones.  *result is, bit for bit, what the composition filter
 * (previous) -> dliom_ndt_target_create, filter (scan) -> dliom_ndt_align gives for the two raw scans and the guess.  A call
 * that fails leaves the matcher as it was.  The scan may be destroyed afterwards.  One thread at a time per matcher, like
 * its context; destroy the matcher before the context. */
typedef struct dliom_ndt_scan_matcher dliom_ndt_scan_matcher;
int dliom_ndt_scan_matcher_create(dliom_ctx* ctx, const dliom_ndt_options* options, float leaf, dliom_ndt_scan_matcher** out);
void dliom_ndt_scan_matcher_destroy(dliom_ndt_scan_matcher* matcher);
int dliom_ndt_scan_matcher_match(dliom_ndt_scan_matcher* matcher, const dliom_cloud* scan, const double* guess16,
                                 dliom_ndt_result* result);
/* *has_target: 1 once a match has succeeded (the matcher holds a scan's cells and the next match writes a result), else 0. */
int dliom_ndt_scan_matcher_has_target(const dliom_ndt_scan_matcher* matcher, int* has_target);

/* Many pairs in one call: the `--method ndt` half of the loop of gen_ground_truth_by_ndt_match.cc:151-261 (:211-222), as
 * dliom_icp_align_batch is its `--method icp` half.  All pairs of a chunk advance in lock step: a round is the next
 * evaluation of every pair still aligning -- at most one launch per kind of evaluation (DLIOM_NDT_EVAL_*) present among
 * them -- and the FINAL ROUND of every pair whose alignment ended in the round before (the final points, the fitness
 * search when the pair has an index, the aligned cloud's norm bound when the clouds are wanted), in ONE launch chain with
 * ONE polled read-back, whatever the number of pairs.  The host decisions between the rounds are those of ALIGNMENT and
 * STEP LENGTH above, pair by pair.
 *
 * Options.  One `options` serves the call; its resolution must be every target's, as dliom_ndt_align demands.  Either step
 * mode.
 *
 * Results.  results[i] is what dliom_ndt_align(pairs[i].target, pairs[i].source, pairs[i].guess, options,
 * pairs[i].fitness_index, ...) returns, bit for bit, in converged, reason, iterations, both evaluation counts, p,
 * transform, score, transformation_probability, fitness_score, fitness_count and pairs.  read_backs of a result is the
 * number of rounds the pair took part in: its evaluations, plus one final round if it has a fitness index or the clouds
 * are wanted.  The batch reads the aligned cloud's norm bound back in the final round's slot, where the single call
 * spends a read-back of its own on it, so this field is ONE LESS than the single call's for a pair that has a fitness
 * index, a non-empty source and a wanted cloud; it is one more for a pair with an empty source, no index and a wanted
 * cloud (the single call reads nothing back for it), and equal otherwise.  The three *_ms fields of a result are 0; the stages'
 * times are in the statistics.  aligned[i] is the single call's cloud, norm bound included.  Results never depend on the
 * limits, on the order of the pairs, or on which other pairs share a chunk.
 *
 * Schedule.  Chunks are consecutive runs of pairs in input order.  A chunk closes when it holds max_pairs_in_flight pairs,
 * or when adding the next pair's dliom_ndt_batch_scratch_bytes(n) would take the chunk's sum above max_scratch_bytes; it
 * always holds at least one pair.  Chunks are not refilled: a chunk takes as many rounds as the pair of it with the most
 * rounds, `steps` is the sum over the chunks, and read_backs == steps.  The default scratch budget holds
 * max_pairs_in_flight = 64 pairs of DLIOM_NDT_BATCH_DEFAULT_POINTS source points: 64 *
 * dliom_ndt_batch_scratch_bytes(65536) = 1 091 354 624 bytes (the leaves of an evaluation alone are 28 doubles a point).
 *
 * Refusals, all before anything runs (DLIOM_ERR_INVALID_ARGUMENT): a NULL context or options; NULL pairs or results
 * with count > 0; count < 0; options that dliom_ndt_align refuses; limits outside their ranges; a pair with a NULL target
 * or source, with a target, a cloud or an index of another context, with a guess that dliom_ndt_align refuses, or with
 * a target whose resolution is not the options'.  count == 0 succeeds and launches nothing.  A HIP or allocation failure
 * fails the whole call and leaves no cloud behind (every aligned[i] is NULL).  There is no per-pair status. */
#define DLIOM_NDT_BATCH_MAX_PAIRS 256
#define DLIOM_NDT_BATCH_DEFAULT_POINTS (64 * 1024)
typedef struct dliom_ndt_pair {
  dliom_ndt_target* target;        /* any number of pairs may name one target */
  const dliom_cloud* source;       /* any number of pairs may name one cloud */
  dliom_nn_index* fitness_index;   /* may be NULL, as in dliom_ndt_align */
  double guess[16];                /* as dliom_ndt_align's guess16 */
} dliom_ndt_pair;
typedef struct dliom_ndt_batch_limits {
  int max_pairs_in_flight;         /* 1 .. DLIOM_NDT_BATCH_MAX_PAIRS; default 64 */
  int reserved;                    /* 0 */
  int64_t max_scratch_bytes;       /* > 0; default 64 * dliom_ndt_batch_scratch_bytes(DLIOM_NDT_BATCH_DEFAULT_POINTS) */
} dliom_ndt_batch_limits;          /* NULL = the defaults, which dliom_ndt_batch_default_limits() returns */
typedef struct dliom_ndt_batch_stats {
  int64_t pairs, chunks, steps;    /* steps: lock-step rounds */
  int64_t read_backs;              /* polled read-backs of the call == steps */
  int64_t synchronizations;        /* stream synchronisations of the call: one a chunk when `aligned` is given (its clouds are
                                      copied out of the chunk's scratch), one for the stages' times while profiling is on */
  int64_t max_in_flight;           /* the largest chunk */
  int64_t pair_evaluations;        /* sum over the results of both evaluation counts */
  int64_t pair_searches;           /* final rounds, summed over the pairs */
  int64_t evaluation_launches[3];  /* by DLIOM_NDT_EVAL_* kind: one a round in which a pair with a non-empty source
                                      evaluates that kind (a kind's list goes in several launches only beyond 2^22 workgroups) */
  int64_t mixed_steps;             /* rounds that launched more than one kind of evaluation, or an evaluation beside a
                                      final round */
  double evaluate_ms, reduce_ms, fitness_ms, host_ms;  /* upload and evaluations | their reductions | the final rounds'
                                      chain | the host's decisions and tables; only while the context's profiling is on */
} dliom_ndt_batch_stats;
int dliom_ndt_batch_default_limits(dliom_ndt_batch_limits* limits);
/* Host only: the device scratch that one pair in flight with source_points points reserves (0 for a negative count). */
int64_t dliom_ndt_batch_scratch_bytes(int64_t source_points);
int dliom_ndt_align_batch(dliom_ctx* ctx, const dliom_ndt_pair* pairs, int count, const dliom_ndt_options* options,
                          const dliom_ndt_batch_limits* limits, dliom_ndt_result* results,
                          dliom_cloud** aligned /* NULL, or count entries */, dliom_ndt_batch_stats* stats /* may be NULL */);

/* Many targets in one call: the other half of that loop, which builds the cells of every distinct target scan before it
 * aligns (gen_ground_truth_by_ndt_match.cc:211-222, setInputTarget).  The clouds of a chunk are treated as ONE
 * concatenation of positions and go through ONE launch chain, whatever their number: the keys, one stable radix sort by
 * key over the whole chunk and one by the target's slot (so that the order is slot, key, ascending point index: within
 * every target dliom_ndt_target_create's), one scan that numbers the chunk's cells, and one launch of the cells' sums, a
 * workgroup a cell over the chunk's total.  The per-cell step (mean, covariance, Jacobi, icov) runs on the host, in
 * double, as in the single build.
 *
 * Results.  out[i] is a dliom_ndt_target like any other: destroyed on its own with dliom_ndt_target_destroy, in any order
 * and before or after its cloud, and usable with dliom_ndt_align, dliom_ndt_evaluate and dliom_ndt_align_batch.  Every cell
 * is, bit for bit, what dliom_ndt_target_create(ctx, clouds[i], options, ...) builds (dliom_ndt_target_cells: index, n,
 * valid, mean, icov), dliom_ndt_target_memory_stats gives the single build's points, kept_points, cells, valid_cells and
 * target_bytes, and the device table of the valid cells is byte-equal to the single build's.  A batch-built target's
 * read_backs is ITS CHUNK'S (2, or 1 for a chunk without any cell) and its build_ms is 0: the stages' times are in the
 * statistics.  A cloud may be named more than once; each mention gets a target of its own.  Results never depend on the
 * limits, on the order of the clouds, or on which other clouds share a chunk.
 *
 * Schedule.  Chunks are consecutive runs of clouds in input order.  A chunk closes when it holds max_targets_in_flight
 * clouds, or when adding the next cloud would take the chunk's point sum above max_points_in_flight; it always holds at
 * least one cloud (a cloud is at most DLIOM_NN_MAX_POINTS points, so positions in a chunk fit an int).  A chunk with at
 * least one cell costs TWO polled read-backs -- every target's cell count and kept count, then the first positions, keys
 * and sums of all its cells -- and a chunk without any cell one; read_backs is the sum over the chunks.  Every chunk takes
 * one upload of its targets' descriptors, the copies of its targets' tables and ONE stream synchronisation at its end
 * (synchronizations == chunks).  The work space is one block on the context, sized before the chain starts for the worst
 * case that every point is a cell of its own: about 108 bytes a point of the largest chunk (scratch_bytes), kept until
 * the context is destroyed.
 *
 * Refusals, all before anything runs (DLIOM_ERR_INVALID_ARGUMENT, no read-back or synchronisation counted on the context):
 * a NULL context, options or out; NULL clouds with count > 0; count < 0; options that dliom_ndt_target_create refuses;
 * limits outside their ranges or reserved != 0; a NULL cloud, a cloud of another context, an empty cloud.  count == 0
 * succeeds and launches nothing.  A HIP or allocation failure fails the whole call, destroys what was built and leaves
 * every out[i] NULL.  There is no per-target status. */
#define DLIOM_NDT_TARGET_BATCH_MAX_TARGETS 256
typedef struct dliom_ndt_target_batch_limits {
  int max_targets_in_flight;       /* 1 .. DLIOM_NDT_TARGET_BATCH_MAX_TARGETS; default 64 */
  int reserved;                    /* 0 */
  int64_t max_points_in_flight;    /* 1 .. 2^30; default 64 * DLIOM_NDT_BATCH_DEFAULT_POINTS */
} dliom_ndt_target_batch_limits;   /* NULL = the defaults, which dliom_ndt_target_batch_default_limits() returns */
typedef struct dliom_ndt_target_batch_stats {
  int64_t targets, chunks;
  int64_t points, kept_points, cells, valid_cells; /* summed over the targets */
  int64_t read_backs;              /* polled read-backs of the call: 2 a chunk with a cell, 1 a chunk without */
  int64_t synchronizations;        /* stream synchronisations of the call: one a chunk */
  int64_t max_in_flight;           /* the largest chunk, in targets */
  int64_t scratch_bytes;           /* the largest chunk's device work space */
  double sort_ms, sums_ms, host_ms, upload_ms; /* keys, both sorts, heads, scan and the first read-back | bounds, the cells'
                                      sums and the second read-back | the per-cell step | the tables' allocations, copies and
                                      the synchronisation; on the host's clock, only while the context's profiling is on */
} dliom_ndt_target_batch_stats;
int dliom_ndt_target_batch_default_limits(dliom_ndt_target_batch_limits* limits);
int dliom_ndt_target_create_batch(dliom_ctx* ctx, const dliom_cloud* const* clouds, int count, const dliom_ndt_options* options,
                                  const dliom_ndt_target_batch_limits* limits, dliom_ndt_target** out /* count entries */,
                                  dliom_ndt_target_batch_stats* stats /* may be NULL */);

/* Kernel timing (HIP events on the context's stream). */
enum {
  DLIOM_KERNEL_RTCSM_SCORE = 0, /* score-volume kernel (dominant) */
  DLIOM_KERNEL_RTCSM_SELECT = 1,
  DLIOM_KERNEL_RTCSM_RESCORE = 2,
  DLIOM_KERNEL_CSM_EVAL = 3,
  DLIOM_KERNEL_INSERT = 4,
  DLIOM_KERNEL_ALLREDUCE = 5,   /* dliom_rtcsm3d_match_sharded_rccl: copy in, ncclAllReduce(max, u64), copy out -- the
                                   collective's own time on this rank's stream, the wait for the slowest peer included */
  DLIOM_KERNEL_PG_HITS = 6,     /* 2D probability grid insertion: end pixels + hit table (the bounds pass included) */
  DLIOM_KERNEL_PG_RAYS = 7,     /* ... the supercover rays (the hot path) */
  DLIOM_KERNEL_PG_CLEAR = 8,    /* ... FinishUpdate over the batch's pixel box */
  DLIOM_KERNEL_COUNT = 9
};
/* enabled: 0 off, 1 every kernel id, otherwise a mask with bit (id + 1) per timed kernel id
 * (2 = the score kernel only: what bench.py's timed region uses; 2 | 64 = score kernel and the sharded match's
 * all-reduce). */
int dliom_ctx_set_profiling(dliom_ctx* ctx, int enabled);
int dliom_ctx_reset_profiling(dliom_ctx* ctx);
int dliom_ctx_kernel_time(dliom_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* DLIOM_H_ */
