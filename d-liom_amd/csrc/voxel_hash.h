// The sparse voxel table of the export stages (outlier.hip, points_xray.hip), device side and host side.
//
// Device side: the extent of a HybridGridBase, the voxel index of one coordinate inside it, keys of up to three 14-bit
// coordinates, and an open-addressing table "64-bit key -> slot" (linear probing) that is filled by compare-and-swap and
// never waited on.  Host side: KeyTable owns the table's three arrays -- keys, slots, and the key of every slot -- and
// grows them between launches (voxel_table.hip): 1024 entries at first, doubled until the load is at most one half, never
// above 2^31 entries; the keys of the slots in use are rehashed into the new arrays, the stream is waited for, and only
// then do the new arrays replace the old ones.  What a slot holds (a leaf of counters, a bit mask, a column's sums) is a
// pool of the stage's own, grown with grown_copy().  A growth that fails at any step frees what it allocated and leaves
// the owner's pointers and capacities as they were.  The read-back of a stage's device words and the flag bits that the
// stages' check kernels share are here as well.
#ifndef DLIOM_CSRC_VOXEL_HASH_H_
#define DLIOM_CSRC_VOXEL_HASH_H_

#include <cstring>

#include "device_common.h"

namespace dliom {

// CHECK_LE(new_bits, 8) (hybrid_grid.h:389): 64 << 8 voxels per axis, indices [-8192, 8191] (hybrid_grid.h:263-268)
constexpr int kMinIndex = -8192, kMaxIndex = 8191;
constexpr uint64_t kEmptyKey = ~uint64_t{0};
constexpr unsigned kNoSlot = 0xFFFFFFFFu;

// ---- keys: 14-bit fields, field 0 least significant, each a coordinate plus a bias that makes it non-negative ---------
constexpr int kKeyBias = -kMinIndex;  // of a voxel coordinate; of a leaf coordinate: kKeyBias >> leaf_bits
__host__ __device__ inline uint64_t key_field(int c, int bias, int i) { return static_cast<uint64_t>(c + bias) << (14 * i); }
constexpr unsigned kKeyMask = 0x3FFFu;  // of one field
__host__ __device__ inline int key_coord(uint64_t key, int i) { return static_cast<int>((key >> (14 * i)) & kKeyMask) - kKeyBias; }
inline void key_xyz(uint64_t key, int32_t* xyz) {  // of a voxel key (z, y, x), z most significant
  for (int i = 0; i < 3; ++i) xyz[i] = key_coord(key, i);
}
// the leaf (a cube of 2^leaf_bits voxels an edge) of a voxel, and the voxel's place in it
__device__ __forceinline__ uint64_t leaf_key(int cx, int cy, int cz, int leaf_bits) {
  const int bias = kKeyBias >> leaf_bits;
  return key_field(cz >> leaf_bits, bias, 2) | key_field(cy >> leaf_bits, bias, 1) | key_field(cx >> leaf_bits, bias, 0);
}
__device__ __forceinline__ int cell_in_leaf(int cx, int cy, int cz, int leaf_bits) {
  const int mask = (1 << leaf_bits) - 1;
  return ((cz & mask) << (2 * leaf_bits)) | ((cy & mask) << leaf_bits) | (cx & mask);
}

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

// ---- host side --------------------------------------------------------------------------------------------------------
struct HashView {  // what a kernel needs of a KeyTable
  uint64_t* keys;  // capacity entries, kEmptyKey: free
  unsigned* slots;
  unsigned mask;  // capacity - 1 (a power of two)
};

// "key -> slot" with the key of every slot; grown on the host while the stream is idle or may be waited for
struct KeyTable {
  uint64_t* keys = nullptr;
  unsigned* slots = nullptr;
  uint64_t* slot_key = nullptr;  // capacity / 2 entries
  int64_t capacity = 0;          // entries, a power of two, at least twice the slots in use
  HashView view() const { return HashView{keys, slots, static_cast<unsigned>(capacity - 1)}; }
  int64_t bytes() const { return capacity * 12 + capacity / 2 * 8; }
  void release() {
    if (keys) (void)hipFree(keys);
    if (slots) (void)hipFree(slots);
    if (slot_key) (void)hipFree(slot_key);
    keys = slot_key = nullptr;
    slots = nullptr;
  }
  // room for `want` slots at a load of at most one half, `used` of them in use; ++*growths unless it is the first
  int grow(dliom_ctx* ctx, int64_t want, int64_t used, int64_t* growths);
};

// *out := a zeroed allocation of `cap` bytes that starts with `used` bytes of `old`.  `old` stays allocated: the caller
// frees it once every array of its group exists.  On failure nothing is left allocated and *out is as it was.
int grown_copy_bytes(dliom_ctx* ctx, const void* old, size_t used, size_t cap, void** out);
template <typename T>
int grown_copy(dliom_ctx* ctx, const T* old, int64_t used, int64_t cap, T** out) {
  return grown_copy_bytes(ctx, old, used * sizeof(T), cap * sizeof(T), reinterpret_cast<void**>(out));
}

// the device words [first, first + count) of a stage on the host
inline int read_words(dliom_ctx* ctx, const unsigned* d_words, int first, int count, unsigned* host) {
  unsigned* pinned = pinned_at<unsigned>(ctx, kPinReadback);
  const GatherJob back{d_words + first, static_cast<unsigned>(count)};
  DLIOM_TRY(gather_and_wait(ctx, &back, 1, pinned));
  std::memcpy(host, pinned, static_cast<size_t>(count) * 4);
  return DLIOM_OK;
}
inline int64_t words64(const unsigned* host, int at) { return static_cast<int64_t>(host[at]) | (static_cast<int64_t>(host[at + 1]) << 32); }

// what the check kernels of the stages flag before anything is written
constexpr unsigned kFlagNonFinite = 1u, kFlagExtent = 2u;
inline int status_of_flag(unsigned flag) {
  if (flag & kFlagNonFinite) return DLIOM_ERR_INVALID_ARGUMENT;
  if (flag & kFlagExtent) return DLIOM_ERR_GRID_EXTENT;
  return DLIOM_OK;
}

}  // namespace dliom

#endif  // DLIOM_CSRC_VOXEL_HASH_H_
