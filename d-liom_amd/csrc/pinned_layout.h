// Layout of a context's page-locked, device-visible staging block (dliom_ctx::pinned, kPinnedBytes, allocated with the
// context) and of the histogram's auxiliary block (dliom_ctx::aux_pinned, kAuxPinnedBytes, made on first use).
//
// Ownership: the block belongs to the entry point that is running.  Every entry point that writes it waits for the
// device before it returns, so the next call finds it free.  Within one call, regions that are live at the same time do
// not overlap: each such group is checked by a static_assert at the end of this file.
//
// Regions that overlap only across time:
//  * the small read-backs at offset 0 (kPinReadback, kPinCsmSums), kPinLmResult and kPinHistogram are each waited for
//    and copied out by the call that issued them, before that call stages anything else;
//  * kPinPoseGraphSums lies inside the bulk regions below (kPinDownload, kPinRtcsmCandidates, kPinFastCsmScores,
//    kPinFrontierUpload): a pose graph call (pose_graph.hip) is an entry point of its own that runs no match, search or
//    download, writes the region once an iteration and has copied it out before it launches anything else or returns;
//  * kPinFeaturePairs and kPinFeatureResults belong to a feature match (feature_match.hip), likewise an entry point of its
//    own: it fills the first before its launches and has copied the second out before it returns;
//  * kPinIcpSums belongs to an alignment or a step of icp.hip, entry points of their own: one read-back an iteration (the
//    sums of the tree reduction), copied out before the next launch.  The index's creation (nn_index.hip) reads its
//    bounding box through kPinReadback, in a call of its own;
//  * kPinIcpBatchReadback and kPinIcpBatchTable belong to a batched alignment (icp_batch.hip), an entry point of its own
//    that runs no single alignment: every lock-step round it fills the table with the descriptors of the pairs in flight
//    before its launches and has copied the pairs' read-back slots out before it writes the table again or returns;
//  * kPinNdtSums belongs to an alignment or an evaluation of ndt.hip, entry points of their own: one read-back an
//    evaluation, copied out before the next launch.  The fitness score at an alignment's end is ICP's (kPinIcpSums); the
//    target's creation and the aligned cloud's norm read a few words through kPinReadback;
//  * kPinNdtBatchReadback and kPinNdtBatchTable belong to a batched NDT alignment (ndt_batch.hip), an entry point of its own
//    that runs no single alignment and no batched ICP alignment (whose regions it lies over): every lock-step round it
//    fills the table with the descriptors of the pairs in flight before its launches and has copied the pairs' read-back
//    slots out before it writes the table again or returns;
//  * kPinNdtTargetBatchTable belongs to a batched NDT target build (ndt_target_batch.hip), an entry point of its own: a
//    chunk fills it with its targets' descriptors before its launches; its one small read-back (a cell count and a kept
//    count a target) goes through kPinReadback and is copied out before the chunk stages anything else.  The cells' first
//    positions, keys and sums are too many for this block: they go to the call's own host memory;
//  * kPinNnIndexBatchTable and kPinNnIndexBatchBoxes belong to a batched index build (nn_index_batch.hip), an entry point
//    of its own that runs no single build: a chunk fills the table with its clouds' descriptors before the boxes' launch,
//    reads every cloud's eight box words back through the second region (8 words x 256 clouds are more than kPinReadback
//    holds), and only then writes the table again, with the grids' views, before the sort's launches.  The chunk's stream
//    synchronisation frees both for the next chunk;
//  * kPinGzipSizes belongs to a launch chain of gzip.hip, which the entry points that compress (dliom_gzip and its kin, the
//    gzipped texture, the framed node records) run only after their own read-backs are copied out: the chain's one
//    read-back, copied out before the chain's download is issued;
//  * the bulk regions from offset 0 (kPinRtcsmCandidates, kPinFastCsmScores, kPinDownload, kPinFrontierUpload) belong
//    to different entry points, except in a fast-CSM search: there device_frontier synchronises and copies its output
//    (kPinFrontierOut) into the score cache before the recursion's device_sums (kPinFastCsmScores) first runs.  The
//    discrete scans' pose upload (kPinPoses) is not waited for when the search skips the frontier; the list that
//    device_sums writes there (16 bytes a candidate from offset 0) reaches into it only beyond 13 312 candidates.
#ifndef DLIOM_CSRC_PINNED_LAYOUT_H_
#define DLIOM_CSRC_PINNED_LAYOUT_H_

#include <cstddef>
#include <initializer_list>

namespace dliom {

constexpr size_t kPinnedBytes = size_t{1} << 20;

struct PinRegion {
  size_t at, bytes;
};

// small read-backs (counts, flags, maxima) of gather_and_wait and the like; the largest, the de-skew stage's, is
// 3 + 976 words
constexpr PinRegion kPinReadback{0, 4096};
// Ceres evaluation (csm3d.hip evaluate): the 28 double sums of one evaluation
constexpr PinRegion kPinCsmSums{0, 1024};
// Ceres in one launch (csm3d.hip): LmKernelOut
constexpr PinRegion kPinLmResult{1024, 1024};
// dliom_cloud_rotational_histogram on the main stream: histogram_size (<= 255) floats and two flag words
constexpr PinRegion kPinHistogram{2048, 2048};
// dliom_cloud_download[_transformed]: packed xyz, in pieces of kPinDownload.bytes / 12 points
constexpr PinRegion kPinDownload{0, kPinnedBytes - 8192};

// an RTCSM match (rtcsm3d.hip)
constexpr PinRegion kPinRtcsmCandidates{0, kPinnedBytes - 81920};  // candidate tables (pageable above this)
constexpr PinRegion kPinBoxTables{kPinnedBytes - 81920, 65536};    // the LDS-box kernel's tables (pageable above this)
constexpr PinRegion kPinSequentialSums{kPinnedBytes - 8192, 4096};  // sequential_probability_sums (sequential_sums.hip): up to 1024 floats
constexpr PinRegion kPinMatchReadback{kPinnedBytes - 4096, 2048};  // [count pair | list | sums | box overflow word]
constexpr PinRegion kPinBoxErrorWord{kPinnedBytes - 2048, 4};      // a shard's box overflow word
constexpr PinRegion kPinRcclWord{kPinnedBytes - 1024, 8};          // the RCCL exchange's 64-bit word

// a single fast-CSM search (fast_csm3d.hip); it also reads kPinSequentialSums back
constexpr PinRegion kPinFastCsmScores{0, kPinnedBytes - 8192};        // device_sums: candidate list, then its sums
constexpr PinRegion kPinFrontierUpload{0, 208 * 1024};                // device_frontier's upload
constexpr PinRegion kPinPoses{208 * 1024, 48 * 1024};                 // the discrete scans' poses (pageable above this)
constexpr PinRegion kPinFrontierOut{256 * 1024, kPinnedBytes - 256 * 1024 - 8192};  // device_frontier's output

// a pose graph solve (pose_graph.hip): the sums of one trust-region iteration, read back once an iteration; while the
// call runs nothing else stages in the block
constexpr PinRegion kPinPoseGraphSums{4096, 256};

// a feature match (feature_match.hip), an entry point of its own like the pose graph's: the pair table it uploads
// (32 bytes a train set) and the one read-back of the call (48 bytes a train set), DLIOM_FEATURE_MAX_TRAIN_SETS of each
constexpr PinRegion kPinFeaturePairs{0, 8192 * 32};
constexpr PinRegion kPinFeatureResults{8192 * 32, 8192 * 48};

// an ICP alignment (icp.hip): the sixteen sums, the count and the search counters of one iteration
constexpr PinRegion kPinIcpSums{4096, 256};

// a batched ICP alignment (icp_batch.hip): a read-back slot (icp_internal.h IcpReadback) for every pair that may be in
// flight (DLIOM_ICP_BATCH_MAX_PAIRS), and the round's upload, a descriptor for each of them
constexpr size_t kPinIcpBatchPairs = 256, kPinIcpBatchSlotBytes = 160, kPinIcpBatchEntryBytes = 384;
constexpr PinRegion kPinIcpBatchReadback{8192, kPinIcpBatchPairs * kPinIcpBatchSlotBytes};
constexpr PinRegion kPinIcpBatchTable{65536, kPinIcpBatchPairs * kPinIcpBatchEntryBytes};

// an NDT evaluation (ndt.hip): up to 28 sums and the pair count
constexpr PinRegion kPinNdtSums{4096 + 256, 256};

// a batched NDT alignment (ndt_batch.hip): a read-back slot for every pair that may be in flight
// (DLIOM_NDT_BATCH_MAX_PAIRS) -- an evaluation's NdtReadback or a final round's IcpReadback -- and the round's upload, a
// descriptor for each of them (the table, the pose's rows, the arrays; in a final round the search's item)
constexpr size_t kPinNdtBatchPairs = 256, kPinNdtBatchSlotBytes = 256, kPinNdtBatchEntryBytes = 1024;
constexpr PinRegion kPinNdtBatchReadback{8192, kPinNdtBatchPairs * kPinNdtBatchSlotBytes};
constexpr PinRegion kPinNdtBatchTable{131072, kPinNdtBatchPairs * kPinNdtBatchEntryBytes};

// a batched NDT target build (ndt_target_batch.hip): the chunk's upload, a descriptor for every target that may be in
// flight (DLIOM_NDT_TARGET_BATCH_MAX_TARGETS); its counts' read-back, two words a target, is kPinReadback
constexpr size_t kPinNdtTargetBatchTargets = 256, kPinNdtTargetBatchEntryBytes = 32;
constexpr PinRegion kPinNdtTargetBatchTable{8192, kPinNdtTargetBatchTargets * kPinNdtTargetBatchEntryBytes};

// a batched index build (nn_index_batch.hip): the chunk's uploads, a descriptor for every cloud that may be in flight
// (DLIOM_NN_INDEX_BATCH_MAX_INDICES), and the boxes' read-back: the clouds' four low words, then their four high words
constexpr size_t kPinNnIndexBatchIndices = 256, kPinNnIndexBatchEntryBytes = 128, kPinNnIndexBatchBoxWords = 8;
constexpr PinRegion kPinNnIndexBatchTable{8192, kPinNnIndexBatchIndices * kPinNnIndexBatchEntryBytes};
constexpr PinRegion kPinNnIndexBatchBoxes{65536, kPinNnIndexBatchIndices * kPinNnIndexBatchBoxWords * 4};

// a launch chain of gzip.hip: [chunks in stored form | the k + 1 offsets of its segments' members], 64 bits each
constexpr PinRegion kPinGzipSizes{0, 65536};

// the auxiliary block: the histogram of dliom_cloud_rotational_histogram_begin / _finish and its completion word
constexpr size_t kAuxPinnedBytes = 4096;
constexpr PinRegion kAuxHistogram{0, 4032};
constexpr PinRegion kAuxDoneWord{4032, 4};

// A region's first byte as a T*, in the context's block or in its auxiliary block (Ctx: dliom_ctx).
template <class T = void, class Ctx>
inline T* pinned_at(Ctx* ctx, PinRegion r) {
  return static_cast<T*>(static_cast<void*>(static_cast<char*>(ctx->pinned) + r.at));
}
template <class T = void, class Ctx>
inline T* aux_pinned_at(Ctx* ctx, PinRegion r) {
  return static_cast<T*>(static_cast<void*>(static_cast<char*>(ctx->aux_pinned) + r.at));
}

constexpr bool pins_inside(std::initializer_list<PinRegion> rs, size_t block) {
  for (const PinRegion& r : rs)
    if (r.at > block || r.bytes > block - r.at) return false;
  return true;
}
constexpr bool pins_disjoint(std::initializer_list<PinRegion> rs) {
  for (const PinRegion* a = rs.begin(); a != rs.end(); ++a)
    for (const PinRegion* b = rs.begin(); b != a; ++b)
      if (a->at < b->at + b->bytes && b->at < a->at + a->bytes) return false;
  return true;
}

static_assert(pins_inside({kPinReadback, kPinCsmSums, kPinLmResult, kPinHistogram, kPinDownload, kPinRtcsmCandidates,
                           kPinBoxTables, kPinSequentialSums, kPinMatchReadback, kPinBoxErrorWord, kPinRcclWord,
                           kPinFastCsmScores, kPinFrontierUpload, kPinPoses, kPinFrontierOut},
                          kPinnedBytes) &&
                  pins_inside({kAuxHistogram, kAuxDoneWord}, kAuxPinnedBytes),
              "every region lies inside its block");
static_assert(pins_disjoint({kPinRtcsmCandidates, kPinBoxTables, kPinSequentialSums, kPinMatchReadback, kPinBoxErrorWord,
                             kPinRcclWord}),
              "an RTCSM match's regions");
static_assert(pins_disjoint({kPinFrontierUpload, kPinPoses, kPinFrontierOut, kPinSequentialSums}),
              "a single fast-CSM search's regions");
static_assert(pins_disjoint({kPinCsmSums, kPinLmResult}), "Ceres' regions");
static_assert(pins_inside({kPinPoseGraphSums}, kPinnedBytes) && pins_disjoint({kPinPoseGraphSums, kPinReadback}),
              "a pose graph solve's region (apart from the small read-backs of the helpers it may call)");
static_assert(pins_inside({kPinFeaturePairs, kPinFeatureResults}, kPinnedBytes) &&
                  pins_disjoint({kPinFeaturePairs, kPinFeatureResults}),
              "a feature match's regions");
static_assert(pins_inside({kPinIcpSums}, kPinnedBytes) && pins_disjoint({kPinIcpSums, kPinReadback}),
              "an ICP alignment's region (apart from the small read-backs of the helpers it may call)");
static_assert(pins_inside({kPinIcpBatchReadback, kPinIcpBatchTable}, kPinnedBytes) &&
                  pins_disjoint({kPinIcpBatchReadback, kPinIcpBatchTable, kPinReadback, kPinIcpSums, kPinNdtSums}),
              "a batched ICP alignment's regions");
static_assert(pins_inside({kPinNdtSums}, kPinnedBytes) && pins_disjoint({kPinNdtSums, kPinIcpSums, kPinReadback}),
              "an NDT alignment's regions (its fitness score is ICP's)");
static_assert(pins_inside({kPinNdtBatchReadback, kPinNdtBatchTable}, kPinnedBytes) &&
                  pins_disjoint({kPinNdtBatchReadback, kPinNdtBatchTable, kPinReadback, kPinIcpSums, kPinNdtSums}),
              "a batched NDT alignment's regions");
static_assert(pins_inside({kPinNdtTargetBatchTable}, kPinnedBytes) && pins_disjoint({kPinNdtTargetBatchTable, kPinReadback}) &&
                  2 * 4 * kPinNdtTargetBatchTargets <= kPinReadback.bytes,
              "a batched NDT target build's regions");
static_assert(pins_inside({kPinNnIndexBatchTable, kPinNnIndexBatchBoxes}, kPinnedBytes) &&
                  pins_disjoint({kPinNnIndexBatchTable, kPinNnIndexBatchBoxes, kPinReadback}) &&
                  kPinNnIndexBatchBoxWords * 4 * kPinNnIndexBatchIndices > kPinReadback.bytes,
              "a batched index build's regions (its boxes would not fit the small read-backs')");
static_assert(pins_inside({kPinGzipSizes}, kPinnedBytes) && kPinGzipSizes.bytes / 8 > 2, "a gzip launch chain's region");
static_assert(pins_disjoint({kAuxHistogram, kAuxDoneWord}), "the auxiliary block's regions");

}  // namespace dliom

#endif  // DLIOM_CSRC_PINNED_LAYOUT_H_
