// Growth of the export stages' sparse voxel tables and of their pools (voxel_hash.h), on the host between launches.
#include <algorithm>

#include "voxel_hash.h"

namespace dliom {
namespace {

constexpr int kBlock = 256;

// the keys of the slots in use into a larger, empty table
__global__ __launch_bounds__(kBlock) void voxel_rehash_kernel(const uint64_t* __restrict__ slot_key, unsigned used, HashView t) {
  const unsigned s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= used) return;
  hash_place(t.keys, t.slots, t.mask, slot_key[s], s);
}

}  // namespace

int KeyTable::grow(dliom_ctx* ctx, int64_t want, int64_t used, int64_t* growths) {
  if (2 * want <= capacity) return DLIOM_OK;
  int64_t cap = std::max<int64_t>(capacity, 1024);
  while (cap < 2 * want) cap <<= 1;
  if (cap > (int64_t{1} << 31)) return DLIOM_ERR_CAPACITY;
  KeyTable t;
  t.capacity = cap;
  hipError_t e = hipMalloc(&t.keys, cap * 8);
  if (e == hipSuccess) e = hipMalloc(&t.slots, cap * 4);
  if (e == hipSuccess) e = hipMalloc(&t.slot_key, cap / 2 * 8);
  if (e == hipSuccess) e = hipMemsetAsync(t.keys, 0xFF, cap * 8, ctx->stream);
  if (e == hipSuccess && used > 0) {
    e = hipMemcpyAsync(t.slot_key, slot_key, used * 8, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(voxel_rehash_kernel, dim3(blocks_of(used, kBlock)), dim3(kBlock), 0, ctx->stream, t.slot_key,
                         static_cast<unsigned>(used), t.view());
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {  // the table stays as it was
    (void)hipStreamSynchronize(ctx->stream);
    t.release();
    set_last_error("KeyTable::grow", e, __FILE__, __LINE__);
    return DLIOM_ERR_HIP;
  }
  release();
  if (capacity > 0) ++*growths;
  *this = t;
  return DLIOM_OK;
}

int grown_copy_bytes(dliom_ctx* ctx, const void* old, size_t used, size_t cap, void** out) {
  char* q = nullptr;
  DLIOM_HIP_TRY(hipMalloc(&q, cap));
  hipError_t e = hipSuccess;
  if (used > 0) e = hipMemcpyAsync(q, old, used, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(q + used, 0, cap - used, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(q);
    set_last_error("grown_copy", e, __FILE__, __LINE__);
    return DLIOM_ERR_HIP;
  }
  *out = q;
  return DLIOM_OK;
}

}  // namespace dliom
