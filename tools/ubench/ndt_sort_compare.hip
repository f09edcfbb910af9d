// The batched NDT target build's sort: K segments of n 64-bit cell keys with 32-bit values (slot << 24 | index),
// put in the order slot, key, index by (a) one stable radix sort by key over the concatenation, one by the slot's bits and a
// gather, as ndt_target_batch.hip does, or (b) one hipcub::DeviceSegmentedRadixSort.  Medians of ten, device events.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 ndt_sort_compare.hip -o ndt_sort_compare; ./ndt_sort_compare [K [n]]
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::printf("error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
__global__ void gather(int total, const int* pos, const unsigned long long* km, const unsigned* vm, unsigned long long* k, int* v) {
  long long at = (long long)blockIdx.x * 256 + threadIdx.x;
  if (at >= total) return;
  int f = pos[at];
  k[at] = km[f];
  v[at] = (int)(vm[f] & 0xffffffu);
}
int main(int argc, char** argv) {
  const int K = argc > 1 ? atoi(argv[1]) : 16, n = argc > 2 ? atoi(argv[2]) : 65536, N = K * n;
  std::vector<unsigned long long> hk(N);
  std::vector<unsigned> hv(N);
  std::vector<int> hi(N), off(K + 1);
  unsigned long long s = 12345;
  for (int i = 0; i < N; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    // about 1400 distinct cells a segment, keys spread over the 63 bits as (z, y, x) cells are
    unsigned long long c = (s >> 33) % 1400;
    hk[i] = ((c / 100 + (1ull << 20)) << 42) | ((c % 100 / 10 + (1ull << 20)) << 21) | (c % 10 + (1ull << 20));
    hv[i] = ((unsigned)(i / n) << 24) | (unsigned)(i % n);
    hi[i] = i;
  }
  for (int k = 0; k <= K; ++k) off[k] = k * n;
  unsigned long long *k_in, *k_mid, *k_out; unsigned *v_in, *v_mid, *v_out; int *iota, *pos, *v_fin, *d_off; void* tmp;
  CK(hipMalloc(&k_in, 8ull * N)); CK(hipMalloc(&k_mid, 8ull * N)); CK(hipMalloc(&k_out, 8ull * N));
  CK(hipMalloc(&v_in, 4ull * N)); CK(hipMalloc(&v_mid, 4ull * N)); CK(hipMalloc(&v_out, 4ull * N));
  CK(hipMalloc(&iota, 4ull * N)); CK(hipMalloc(&pos, 4ull * N)); CK(hipMalloc(&v_fin, 4ull * N)); CK(hipMalloc(&d_off, 4 * (K + 1)));
  CK(hipMemcpy(k_in, hk.data(), 8ull * N, hipMemcpyHostToDevice)); CK(hipMemcpy(v_in, hv.data(), 4ull * N, hipMemcpyHostToDevice));
  CK(hipMemcpy(iota, hi.data(), 4ull * N, hipMemcpyHostToDevice)); CK(hipMemcpy(d_off, off.data(), 4 * (K + 1), hipMemcpyHostToDevice));
  int bits = 0; while ((1 << bits) < K) ++bits;
  size_t b1 = 0, b2 = 0, b3 = 0;
  CK(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, k_in, k_mid, v_in, v_mid, N, 0, 64));
  CK(hipcub::DeviceRadixSort::SortPairs(nullptr, b2, v_mid, v_out, iota, pos, N, 24, 24 + std::max(bits, 1)));
  CK(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, b3, k_in, k_out, v_in, v_out, N, K, d_off, d_off + 1, 0, 64));
  size_t tb = std::max(b1, std::max(b2, b3));
  CK(hipMalloc(&tmp, tb));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  std::vector<float> two, seg;
  for (int r = 0; r < 12; ++r) {
    float ms;
    CK(hipEventRecord(e0));
    CK(hipcub::DeviceRadixSort::SortPairs(tmp, b1, k_in, k_mid, v_in, v_mid, N, 0, 64));
    if (K > 1) {
      CK(hipcub::DeviceRadixSort::SortPairs(tmp, b2, v_mid, v_out, iota, pos, N, 24, 24 + bits));
      gather<<<(N + 255) / 256, 256>>>(N, pos, k_mid, v_mid, k_out, v_fin);
    }
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 2) two.push_back(ms);
    CK(hipEventRecord(e0));
    CK(hipcub::DeviceSegmentedRadixSort::SortPairs(tmp, b3, k_in, k_out, v_in, v_out, N, K, d_off, d_off + 1, 0, 64));
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 2) seg.push_back(ms);
  }
  std::sort(two.begin(), two.end()); std::sort(seg.begin(), seg.end());
  std::printf("{\"segments\": %d, \"points_a_segment\": %d, \"two_sorts_and_gather_ms\": %.4f, \"segmented_sort_ms\": %.4f}\n", K, n, two[two.size() / 2], seg[seg.size() / 2]);
  return 0;
}
