// What the sparse voxel tables of the export stages share (outlier.hip, points_xray.hip): the extent of a
// HybridGridBase, the voxel index of one coordinate inside it, and an open-addressing table "64-bit key -> slot" that is
// filled by compare-and-swap, never waited on, and grown on the host between launches.
#ifndef DLIOM_CSRC_VOXEL_HASH_H_
#define DLIOM_CSRC_VOXEL_HASH_H_

#include "device_common.h"

namespace dliom {

// CHECK_LE(new_bits, 8) (hybrid_grid.h:389): 64 << 8 voxels per axis, indices [-8192, 8191] (hybrid_grid.h:263-268)
constexpr int kMinIndex = -8192, kMaxIndex = 8191;
constexpr uint64_t kEmptyKey = ~uint64_t{0};
constexpr unsigned kNoSlot = 0xFFFFFFFFu;

__host__ __device__ inline unsigned hash_key(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return static_cast<unsigned>(k);
}

// GetCellIndex of one coordinate (hybrid_grid.h:430-434) where the result is a voxel the grid can hold; false
// otherwise (and for NaN).  |q| < 16384 keeps the conversion to int defined.
__device__ __forceinline__ bool cell_in_extent(float p, float resolution, int* cell) {
  const float q = p / resolution;
  if (!(fabsf(q) < 16384.f)) return false;
  const int c = lround_away(q);
  *cell = c;
  return c >= kMinIndex && c <= kMaxIndex;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) <= 3.4028234e38f && fabsf(y) <= 3.4028234e38f && fabsf(z) <= 3.4028234e38f;  // false for NaN
}

// slot of `key`, kNoSlot if the table has none; *probes += entries read.  Ends: the table is at most half full.
__device__ __forceinline__ unsigned hash_find(const uint64_t* keys, const unsigned* slots, unsigned mask, uint64_t key,
                                              unsigned* probes) {
  unsigned h = hash_key(key) & mask;
  for (;;) {
    const uint64_t k = keys[h];
    ++*probes;
    if (k == key) return slots[h];
    if (k == kEmptyKey) return kNoSlot;
    h = (h + 1u) & mask;
  }
}

// `key` into the table if it is not there: claimed with one compare-and-swap, its slot taken from *counter by the
// winner, who also notes the key of the slot.  Nothing waits for another thread: slots[] of a key claimed in this launch
// is read by the next launch only.
__device__ __forceinline__ void hash_claim(uint64_t* keys, unsigned* slots, unsigned mask, uint64_t key, unsigned* counter,
                                           uint64_t* slot_key) {
  unsigned h = hash_key(key) & mask;
  for (;;) {
    uint64_t k = keys[h];
    if (k == kEmptyKey) {
      k = atomicCAS(reinterpret_cast<unsigned long long*>(&keys[h]), static_cast<unsigned long long>(kEmptyKey),
                    static_cast<unsigned long long>(key));
      if (k == kEmptyKey) {
        const unsigned slot = atomicAdd(counter, 1u);
        slots[h] = slot;
        slot_key[slot] = key;
        return;
      }
    }
    if (k == key) return;
    h = (h + 1u) & mask;
  }
}

// the key of slot `s` into a larger, empty table (every key once)
__device__ __forceinline__ void hash_place(uint64_t* keys, unsigned* slots, unsigned mask, uint64_t key, unsigned s) {
  unsigned h = hash_key(key) & mask;
  for (;;) {
    if (keys[h] == kEmptyKey &&
        atomicCAS(reinterpret_cast<unsigned long long*>(&keys[h]), static_cast<unsigned long long>(kEmptyKey),
                  static_cast<unsigned long long>(key)) == static_cast<unsigned long long>(kEmptyKey)) {
      slots[h] = s;
      return;
    }
    h = (h + 1u) & mask;
  }
}

}  // namespace dliom

#endif  // DLIOM_CSRC_VOXEL_HASH_H_
