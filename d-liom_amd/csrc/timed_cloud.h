// dliom_timed_cloud (dliom.h "PointCloud2 messages decoded on the device"): the object point_cloud2.hip makes of a message
// and range_sync.hip makes of two of them.
#ifndef DLIOM_CSRC_TIMED_CLOUD_H_
#define DLIOM_CSRC_TIMED_CLOUD_H_

#include "internal.h"

struct dliom_timed_cloud {
  dliom_ctx* ctx = nullptr;
  int device = 0;
  int64_t n = 0;
  void* base = nullptr;  // a block of the cloud pool: xyzt | intensities or origin index (null: the empty object)
  size_t base_bytes = 0;
  float4* d_xyzt = nullptr;
  float* d_intensities = nullptr;  // null: none (the SLAM modes)
  bool has_intensities = false;    // "one a point", also of an empty object made by an export mode
  float* d_origin_index = nullptr;  // null: none (everything but a merge's result)
  bool has_origin_index = false;    // "one a point", as above
  float front_t = 0.f, back_t = 0.f;
};

#endif  // DLIOM_CSRC_TIMED_CLOUD_H_
