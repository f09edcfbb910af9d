// Submap image features (dliom.h "submap image features"): cv::threshold, cv::erode and SURF::detectAndCompute of
// ConstraintBuilder3D::ExtractFeaturesForSubmap (constraint_builder_3d.cc:451-458) on an image in HBM.  The definition --
// the templates, the written order of every float and double operation, the integer patch -- is stated once, in the
// header; the kernels below follow it operation for operation (this file is built with -ffp-contract=off and correctly
// rounded division and sqrtf like every other).  No floating-point atomics; integer atomics count the candidates and
// add the patch's exact integer sums in LDS.
//
//   surf_binarize_erode_kernel  16 x 16 pixels a workgroup: the binarised tile and its halo in LDS, the k x k minimum
//   surf_row_scan_kernel        a workgroup an image row: prefix sums (wave scans and a carry) into S's row y + 1
//   surf_column_scan_kernel     a lane a column of S: the running sum down the rows (coalesced across the wave)
//   surf_layer_kernel           blockIdx.y = (octave, layer): the ten resized boxes in LDS, a lane an array position
//   surf_maxima_kernel          blockIdx.y = (octave, middle layer): a lane a position; threshold, 26 neighbours, the
//                               refinement in double; a kept candidate takes a slot with one integer atomic
//   hipcub radix sort           64-bit keys (~response bits, generation index): unique, so the slot order is forgotten
//   surf_orientation_kernel     a wavefront a key point: samples compacted in order into LDS (ballot), a lane a window
//                               running the sequential sums, a 64-bit max of (mod bits, ~window) across the wave
//   surf_compact_kernel         one wavefront: the surviving key points in order (ballot prefix) and their number
//   surf_descriptor_kernel      a workgroup of 1024 a key point: the 21 x 21 integer patch in LDS (an item a (patch pixel,
//                               window row), the rotated window read straight from the eroded image, the rows' exact
//                               integer shares added in LDS), the 400 gradient pairs, a lane a (sub-region, component)
//                               for the 25 sequential adds, one lane for the norm
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "internal.h"

namespace dliom {
namespace {

constexpr int kTile = 16;
constexpr int kMaxK = DLIOM_SURF_MAX_STRUCTURE_ELEMENT;
constexpr int kMaxKeypoints = DLIOM_SURF_MAX_KEYPOINTS;
constexpr int kOriSamples = DLIOM_SURF_ORI_SAMPLES;
constexpr int kOriWindows = 72;
constexpr int kPatch = DLIOM_SURF_PATCH;  // 20 gradient rows; the patch itself is 21 x 21
constexpr int kMaxLayers = 4 * 5;
constexpr int kDescriptorThreads = 1024;
constexpr int kRecordFloats = 8;  // a candidate: the seven floats of a key point and a pad

// the templates are the header's: its macros initialise these tables and nothing else writes the numbers out
__constant__ int kDxx[3][5] = DLIOM_SURF_TEMPLATE_DXX;
__constant__ int kDyy[3][5] = DLIOM_SURF_TEMPLATE_DYY;
__constant__ int kDxy[4][5] = DLIOM_SURF_TEMPLATE_DXY;
__constant__ int kWaveletX[2][5] = DLIOM_SURF_WAVELET_X;
__constant__ int kWaveletY[2][5] = DLIOM_SURF_WAVELET_Y;

struct Box {
  int x1, y1, x2, y2;
  float w;
};

// the Gaussian tables and the orientation offsets, made on the host when the library is loaded (dliom.h step 6)
struct SurfTables {
  float g[2 * DLIOM_SURF_ORI_RADIUS + 1];
  float h[DLIOM_SURF_PATCH];
  int oi[kOriSamples], oj[kOriSamples];
  SurfTables() {
    gaussian(g, 2 * DLIOM_SURF_ORI_RADIUS + 1, DLIOM_SURF_ORI_SIGMA);
    gaussian(h, DLIOM_SURF_PATCH, DLIOM_SURF_DESCRIPTOR_SIGMA);
    int n = 0;
    const int R = DLIOM_SURF_ORI_RADIUS;
    for (int i = -R; i <= R; ++i)
      for (int j = -R; j <= R; ++j)
        if (i * i + j * j <= R * R && n < kOriSamples) {
          oi[n] = i;
          oj[n] = j;
          ++n;
        }
    for (; n < kOriSamples; ++n) oi[n] = oj[n] = 0;
  }
  static void gaussian(float* out, int n, double sigma) {
    double t[32];
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
      const double x = i - (n - 1) * 0.5;
      t[i] = std::exp(-(x * x) / (2.0 * sigma * sigma));
      sum += t[i];
    }
    for (int i = 0; i < n; ++i) out[i] = static_cast<float>(t[i] / sum);
  }
};
const SurfTables kHostTables;

struct SurfLayer {
  int size, step, rows, cols, samples_i, samples_j, m, pad;
  long long offset;  // of the layer's arrays in det / trace, in floats
};
struct SurfLayerTable {
  int octaves, layers;  // layers an octave: n_octave_layers + 2; entry = octave * layers + layer
  SurfLayer L[kMaxLayers];
};

__device__ inline Box resize_box(const int* src, float ratio) {
  Box b;
  b.x1 = static_cast<int>(rintf(ratio * static_cast<float>(src[0])));
  b.y1 = static_cast<int>(rintf(ratio * static_cast<float>(src[1])));
  b.x2 = static_cast<int>(rintf(ratio * static_cast<float>(src[2])));
  b.y2 = static_cast<int>(rintf(ratio * static_cast<float>(src[3])));
  b.w = static_cast<float>(src[4]) / static_cast<float>((b.x2 - b.x1) * (b.y2 - b.y1));
  return b;
}

// S: (H + 1) x (W + 1), stride = W + 1
__device__ inline float box_response(const int* __restrict__ S, int stride, int x0, int y0, const Box* boxes, int n) {
  float r = 0.f;
  for (int k = 0; k < n; ++k) {
    const Box b = boxes[k];
    const int* top = S + static_cast<size_t>(y0 + b.y1) * stride + x0;
    const int* bottom = S + static_cast<size_t>(y0 + b.y2) * stride + x0;
    const unsigned sum = static_cast<unsigned>(top[b.x1]) + static_cast<unsigned>(bottom[b.x2]) -
                         static_cast<unsigned>(bottom[b.x1]) - static_cast<unsigned>(top[b.x2]);
    r = r + static_cast<float>(static_cast<int>(sum)) * b.w;
  }
  return r;
}

// ---- step 1 --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void surf_binarize_erode_kernel(const uint8_t* __restrict__ in, int W, int H, int threshold,
                                                                  int k, uint8_t* __restrict__ out) {
  __shared__ uint8_t tile[(kTile + kMaxK - 1) * (kTile + kMaxK - 1)];
  const int a = k / 2, side = kTile + k - 1;
  const int x0 = static_cast<int>(blockIdx.x) * kTile - a, y0 = static_cast<int>(blockIdx.y) * kTile - a;
  for (int e = threadIdx.x; e < side * side; e += 256) {
    const int x = x0 + e % side, y = y0 + e / side;
    uint8_t v = 255;  // outside the image: no part in a minimum over {0, 255}
    if (x >= 0 && x < W && y >= 0 && y < H) v = in[static_cast<size_t>(y) * W + x] > threshold ? 255 : 0;
    tile[e] = v;
  }
  __syncthreads();
  const int lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;
  const int x = static_cast<int>(blockIdx.x) * kTile + lx, y = static_cast<int>(blockIdx.y) * kTile + ly;
  if (x >= W || y >= H) return;
  int m = 255;
  for (int dy = 0; dy < k; ++dy)
    for (int dx = 0; dx < k; ++dx) m = min(m, static_cast<int>(tile[(ly + dy) * side + lx + dx]));
  out[static_cast<size_t>(y) * W + x] = static_cast<uint8_t>(m);
}

// ---- step 2 --------------------------------------------------------------------------------------------------------
// workgroup 0 clears S's row 0; workgroup y + 1 writes the prefix sums of image row y into S's row y + 1
__global__ __launch_bounds__(256) void surf_row_scan_kernel(const uint8_t* __restrict__ img, int W, int* __restrict__ S) {
  __shared__ int wave_total[4];
  const int stride = W + 1;
  if (blockIdx.x == 0) {
    for (int x = threadIdx.x; x < stride; x += 256) S[x] = 0;
    return;
  }
  const int y = static_cast<int>(blockIdx.x) - 1;
  int* const row = S + static_cast<size_t>(y + 1) * stride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) row[0] = 0;
  int carry = 0;
  for (int base = 0; base < W; base += 256) {
    const int x = base + threadIdx.x;
    int v = x < W ? img[static_cast<size_t>(y) * W + x] : 0;
    for (int off = 1; off < 64; off <<= 1) {
      const int other = __shfl_up(v, off);
      if (lane >= off) v += other;
    }
    if (lane == 63) wave_total[wave] = v;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before += wave_total[w];
    if (x < W) row[x + 1] = before + v;
    carry += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    __syncthreads();
  }
}

// The loads of a group of rows are issued together and the running sum is applied afterwards: one memory latency a
// group instead of one a row (integers: the order is free).
__global__ __launch_bounds__(256) void surf_column_scan_kernel(int W, int H, int* __restrict__ S) {
  constexpr int kRows = 16;
  const int x = static_cast<int>(blockIdx.x) * 256 + threadIdx.x + 1;
  if (x > W) return;
  const size_t stride = static_cast<size_t>(W) + 1;
  int acc = 0;
  for (int y0 = 1; y0 <= H; y0 += kRows) {
    int* const p = S + static_cast<size_t>(y0) * stride + x;
    int v[kRows];
#pragma unroll
    for (int u = 0; u < kRows; ++u) v[u] = y0 + u <= H ? p[u * stride] : 0;
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      acc += v[u];
      if (y0 + u <= H) p[u * stride] = acc;
    }
  }
}

// ---- step 3 --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void surf_layer_kernel(const int* __restrict__ S, int W, SurfLayerTable T, float* __restrict__ det,
                                                         float* __restrict__ trace) {
  __shared__ Box boxes[10];
  const SurfLayer L = T.L[blockIdx.y];
  const long long cells = static_cast<long long>(L.rows) * L.cols;
  if (static_cast<long long>(blockIdx.x) * 256 >= cells) return;  // the whole workgroup
  if (threadIdx.x < 10) {  // boxes 0-2: Dxx, 3-5: Dyy, 6-9: Dxy
    const int t = threadIdx.x;
    boxes[t] = resize_box(t < 3 ? kDxx[t] : t < 6 ? kDyy[t - 3] : kDxy[t - 6], static_cast<float>(L.size) / 9.0f);
  }
  __syncthreads();
  const long long p = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (p >= cells) return;
  const int i = static_cast<int>(p / L.cols) - L.m, j = static_cast<int>(p % L.cols) - L.m;
  float d = 0.f, t = 0.f;
  if (i >= 0 && i < L.samples_i && j >= 0 && j < L.samples_j) {
    const float dxx = box_response(S, W + 1, j * L.step, i * L.step, boxes, 3);
    const float dyy = box_response(S, W + 1, j * L.step, i * L.step, boxes + 3, 3);
    const float dxy = box_response(S, W + 1, j * L.step, i * L.step, boxes + 6, 4);
    d = dxx * dyy - (0.81f * dxy) * dxy;
    t = dxx + dyy;
  }
  det[L.offset + p] = d;
  trace[L.offset + p] = t;
}

// ---- step 4 --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void surf_maxima_kernel(SurfLayerTable T, const float* __restrict__ det,
                                                          const float* __restrict__ trace, float threshold,
                                                          unsigned* __restrict__ counter, unsigned long long* __restrict__ keys,
                                                          unsigned* __restrict__ slots, float* __restrict__ records) {
  const int middle = T.layers - 2;
  const int o = static_cast<int>(blockIdx.y) / middle, l = 1 + static_cast<int>(blockIdx.y) % middle;
  const SurfLayer L = T.L[o * T.layers + l];
  const int above_size = T.L[o * T.layers + l + 1].size, below_size = T.L[o * T.layers + l - 1].size;
  const int margin = (above_size / 2) / L.step + 1;
  const int span_i = L.rows - 2 * margin, span_j = L.cols - 2 * margin;
  if (span_i <= 0 || span_j <= 0) return;
  const long long p = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (p >= static_cast<long long>(span_i) * span_j) return;
  const int i = margin + static_cast<int>(p / span_j), j = margin + static_cast<int>(p % span_j);
  const float* const dl[3] = {det + T.L[o * T.layers + l - 1].offset, det + L.offset, det + T.L[o * T.layers + l + 1].offset};
  const float v = dl[1][static_cast<size_t>(i) * L.cols + j];
  if (!(v > threshold)) return;
  float N[3][3][3];
  bool greatest = true;
  for (int s = 0; s < 3; ++s)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const float n = dl[s][static_cast<size_t>(i + r - 1) * L.cols + (j + c - 1)];
        N[s][r][c] = n;
        if (!(s == 1 && r == 1 && c == 1) && !(v > n)) greatest = false;
      }
  if (!greatest) return;
#define NB(s, r, c) N[(s) + 1][(r) + 1][(c) + 1]
  const float bx = -((NB(0, 0, 1) - NB(0, 0, -1)) * 0.5f), by = -((NB(0, 1, 0) - NB(0, -1, 0)) * 0.5f),
              bs = -((NB(1, 0, 0) - NB(-1, 0, 0)) * 0.5f);
  const float axx = (NB(0, 0, -1) - 2.f * v) + NB(0, 0, 1), ayy = (NB(0, -1, 0) - 2.f * v) + NB(0, 1, 0),
              ass = (NB(-1, 0, 0) - 2.f * v) + NB(1, 0, 0);
  const float axy = (((NB(0, 1, 1) - NB(0, 1, -1)) - NB(0, -1, 1)) + NB(0, -1, -1)) * 0.25f;
  const float axs = (((NB(1, 0, 1) - NB(1, 0, -1)) - NB(-1, 0, 1)) + NB(-1, 0, -1)) * 0.25f;
  const float ays = (((NB(1, 1, 0) - NB(1, -1, 0)) - NB(-1, 1, 0)) + NB(-1, -1, 0)) * 0.25f;
#undef NB
  const double a = axx, b = axy, c = axs, d = ayy, e = ays, f = ass, pp = bx, q = by, r = bs;
  const double c00 = d * f - e * e, c01 = b * f - c * e, c02 = b * e - c * d;
  const double D = (a * c00 - b * c01) + c * c02;
  if (D == 0.0) return;
  const double qfer = q * f - e * r, qedr = q * e - d * r, brqc = b * r - q * c;
  const float t0 = static_cast<float>(((pp * c00 - b * qfer) + c * qedr) / D);
  const float t1 = static_cast<float>(((a * qfer - pp * c01) + c * brqc) / D);
  const float t2 = static_cast<float>(((a * (d * r - q * e) - b * brqc) + pp * c02) / D);
  if (!((t0 != 0.f || t1 != 0.f || t2 != 0.f) && fabsf(t0) <= 1.f && fabsf(t1) <= 1.f && fabsf(t2) <= 1.f)) return;
  const unsigned slot = atomicAdd(counter, 1u);
  if (slot >= static_cast<unsigned>(kMaxKeypoints)) return;
  const float centre = static_cast<float>(L.size - 1) * 0.5f, step = static_cast<float>(L.step);
  const float tr = trace[L.offset + static_cast<size_t>(i) * L.cols + j];
  float* const rec = records + static_cast<size_t>(slot) * kRecordFloats;
  rec[0] = (static_cast<float>(L.step * (j - L.m)) + centre) + t0 * step;
  rec[1] = (static_cast<float>(L.step * (i - L.m)) + centre) + t1 * step;
  rec[2] = rintf(static_cast<float>(L.size) + t2 * static_cast<float>(L.size - below_size));
  rec[3] = -1.f;
  rec[4] = v;
  rec[5] = static_cast<float>(o);
  rec[6] = static_cast<float>((tr > 0.f ? 1 : 0) - (tr < 0.f ? 1 : 0));
  rec[7] = 0.f;
  const unsigned generation = (static_cast<unsigned>(o) << 25) | (static_cast<unsigned>(l) << 23) | static_cast<unsigned>(i * L.cols + j);
  keys[slot] = (static_cast<unsigned long long>(~__float_as_uint(v)) << 32) | generation;
  slots[slot] = slot;
}

// ---- step 6 --------------------------------------------------------------------------------------------------------
__device__ inline float fast_atan2(float y, float x) {
  const float scale = static_cast<float>(180.0 / 3.14159265358979323846);
  const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale, p5 = 0.1555786518463281f * scale,
              p7 = -0.04432655554792128f * scale;
  const float ax = fabsf(x), ay = fabsf(y);
  const float c = fminf(ax, ay) / (fmaxf(ax, ay) + static_cast<float>(DBL_EPSILON));
  const float c2 = c * c;
  float a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  if (ax < ay) a = 90.f - a;
  if (x < 0.f) a = 180.f - a;
  if (y < 0.f) a = 360.f - a;
  return a;
}

// ori[k] = (angle, cos, sin, kept ? 1 : 0) of the k-th key point in sorted order
__global__ __launch_bounds__(64) void surf_orientation_kernel(const int* __restrict__ S, int W, int H,
                                                              const float* __restrict__ records,
                                                              const unsigned* __restrict__ sorted_slots,
                                                              const SurfTables* __restrict__ tables, float4* __restrict__ ori) {
  __shared__ float X[kOriSamples], Y[kOriSamples], sumx[kOriWindows], sumy[kOriWindows];
  __shared__ int A[kOriSamples];
  __shared__ Box wavelets[4];
  const int lane = threadIdx.x;
  const float* const rec = records + static_cast<size_t>(sorted_slots[blockIdx.x]) * kRecordFloats;
  const float kx = rec[0], ky = rec[1];
  const float s = rec[2] * 1.2f / 9.0f;
  const int side = 2 * static_cast<int>(rintf(2.f * s));
  if (H + 1 < side || W + 1 < side) {  // the whole wavefront
    if (lane == 0) ori[blockIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  if (lane < 4) wavelets[lane] = resize_box(lane < 2 ? kWaveletX[lane] : kWaveletY[lane - 2], static_cast<float>(side) / 4.0f);
  __syncthreads();
  const float half = static_cast<float>(side - 1) / 2.f;
  int n = 0;
  for (int base = 0; base < kOriSamples; base += 64) {
    const int kk = base + lane;
    bool ok = false;
    float vx = 0.f, vy = 0.f;
    if (kk < kOriSamples) {
      const int i = tables->oi[kk], j = tables->oj[kk];
      const int px = static_cast<int>(rintf((kx + static_cast<float>(i) * s) - half));
      const int py = static_cast<int>(rintf((ky + static_cast<float>(j) * s) - half));
      ok = py >= 0 && py < H + 1 - side && px >= 0 && px < W + 1 - side;
      if (ok) {
        const float weight = tables->g[i + DLIOM_SURF_ORI_RADIUS] * tables->g[j + DLIOM_SURF_ORI_RADIUS];
        vx = box_response(S, W + 1, px, py, wavelets, 2) * weight;
        vy = box_response(S, W + 1, px, py, wavelets + 2, 2) * weight;
      }
    }
    const unsigned long long votes = __ballot(ok);
    if (ok) {
      const int at = n + __popcll(votes & ((1ull << lane) - 1ull));
      X[at] = vx;
      Y[at] = vy;
      A[at] = static_cast<int>(rintf(fast_atan2(vy, vx)));
    }
    n += __popcll(votes);
  }
  __syncthreads();
  if (n == 0) {
    if (lane == 0) ori[blockIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  unsigned long long best = 0;  // mod bits << 32 | ~window; mod >= +0, so its bits order as its value
  for (int w = lane; w < kOriWindows; w += 64) {
    const int angle = 5 * w;
    float sx = 0.f, sy = 0.f;
    for (int m = 0; m < n; ++m) {
      const int d = abs(A[m] - angle);
      if (d < 30 || d > 330) {
        sx = sx + X[m];
        sy = sy + Y[m];
      }
    }
    sumx[w] = sx;
    sumy[w] = sy;
    const float mod = sx * sx + sy * sy;
    const unsigned long long key = (static_cast<unsigned long long>(__float_as_uint(mod)) << 32) | (0xFFFFFFFFu - static_cast<unsigned>(w));
    best = key > best ? key : best;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(best, off);
    best = other > best ? other : best;
  }
  __syncthreads();
  if (lane != 0) return;
  float4 result = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((best >> 32) != 0) {  // a window above 0
    const int w = static_cast<int>(0xFFFFFFFFu - static_cast<unsigned>(best & 0xFFFFFFFFull));
    const float bestx = sumx[w], besty = sumy[w];
    const float norm = sqrtf(bestx * bestx + besty * besty);
    if (norm != 0.f) result = make_float4(fast_atan2(-besty, bestx), bestx / norm, besty / norm, 1.f);
  }
  ori[blockIdx.x] = result;
}

// ---- step 8 --------------------------------------------------------------------------------------------------------
// one wavefront: keypoints (7 floats) and frames (cos, sin) of the kept key points in order; *count = their number
__global__ __launch_bounds__(64) void surf_compact_kernel(const float* __restrict__ records, const unsigned* __restrict__ sorted_slots,
                                                          const float4* __restrict__ ori, int n, float* __restrict__ keypoints,
                                                          float2* __restrict__ frames, unsigned* __restrict__ count) {
  const int lane = threadIdx.x;
  int kept = 0;
  for (int base = 0; base < n; base += 64) {
    const int k = base + lane;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < n) o = ori[k];
    const bool keep = o.w != 0.f;
    const unsigned long long votes = __ballot(keep);
    if (keep) {
      const int at = kept + __popcll(votes & ((1ull << lane) - 1ull));
      const float* const rec = records + static_cast<size_t>(sorted_slots[k]) * kRecordFloats;
      float* const out = keypoints + static_cast<size_t>(at) * DLIOM_SURF_KEYPOINT_FLOATS;
      out[0] = rec[0];
      out[1] = rec[1];
      out[2] = rec[2];
      out[3] = o.x;
      out[4] = rec[4];
      out[5] = rec[5];
      out[6] = rec[6];
      frames[at] = make_float2(o.y, o.z);
    }
    kept += __popcll(votes);
  }
  if (lane == 0) *count = static_cast<unsigned>(kept);
}

// ---- step 7 --------------------------------------------------------------------------------------------------------
// Sums stay below 2^31: size <= 264 (octave 3, layer 3, offset 1), so w <= 739 and 2 * 255 * w * w + w * w < 2^29.
__global__ __launch_bounds__(kDescriptorThreads) void surf_descriptor_kernel(const uint8_t* __restrict__ img, int W, int H,
                                                              const float* __restrict__ keypoints, const float2* __restrict__ frames,
                                                              const unsigned* __restrict__ count,
                                                              const SurfTables* __restrict__ tables, float* __restrict__ descriptors) {
  constexpr int P = kPatch + 1;
  __shared__ int patch[P * P];
  __shared__ float DX[kPatch * kPatch], DY[kPatch * kPatch], vec[64];
  __shared__ float scale;
  if (blockIdx.x >= *count) return;  // the whole workgroup
  const float* const kp = keypoints + static_cast<size_t>(blockIdx.x) * DLIOM_SURF_KEYPOINT_FLOATS;
  const float kx = kp[0], ky = kp[1];
  const float s = kp[2] * 1.2f / 9.0f;
  const float2 frame = frames[blockIdx.x];
  const float c = frame.x, sn = frame.y;
  const int w = static_cast<int>(static_cast<float>(P) * s);
  const float off = -(static_cast<float>(w - 1) / 2.f);
  const float start_x = (kx + off * c) + off * sn;
  const float start_y = (ky - off * sn) + off * c;
  // the window's area sums: an item is (patch pixel, one of the window rows under it); the rows' integer shares meet in
  // LDS with integer atomics (exact, so their order is free)
  for (int e = threadIdx.x; e < P * P; e += kDescriptorThreads) patch[e] = 0;
  __syncthreads();
  const int rows_a_pixel = w / P + 2;  // window rows that can overlap one patch row
  for (int item = threadIdx.x; item < P * P * rows_a_pixel; item += kDescriptorThreads) {
    const int e = item / rows_a_pixel, pi = e / P, pj = e % P;
    const int ki = (w * pi) / P + item % rows_a_pixel;
    if (ki * P >= w * (pi + 1)) continue;
    const int oi = min(P * ki + P, w * (pi + 1)) - max(P * ki, w * pi);
    const float row_x = start_x + static_cast<float>(ki) * sn, row_y = start_y + static_cast<float>(ki) * c;
    const int end = w * (pj + 1);
    int row = 0;
    for (int kj = (w * pj) / P; kj * P < end; kj += 4) {
      int v[4], oj[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // four loads in flight; a column beyond the pixel has overlap 0 (its address is clamped like any)
        const int k = kj + u;
        oj[u] = max(min(P * k + P, end) - max(P * k, w * pj), 0);
        const float px = row_x + static_cast<float>(k) * c, py = row_y - static_cast<float>(k) * sn;
        const int x = min(max(static_cast<int>(rintf(px)), 0), W - 1), y = min(max(static_cast<int>(rintf(py)), 0), H - 1);
        v[u] = img[static_cast<size_t>(y) * W + x];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) row += oj[u] * v[u];
    }
    atomicAdd(&patch[e], oi * row);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < P * P; e += kDescriptorThreads) patch[e] = (2 * patch[e] + w * w) / (2 * w * w);
  __syncthreads();
  for (int e = threadIdx.x; e < kPatch * kPatch; e += kDescriptorThreads) {
    const int i = e / kPatch, j = e % kPatch;
    const float dw = tables->h[i] * tables->h[j];
    const int p00 = patch[i * P + j], p01 = patch[i * P + j + 1], p10 = patch[(i + 1) * P + j], p11 = patch[(i + 1) * P + j + 1];
    DX[e] = static_cast<float>(p01 - p00 + p11 - p10) * dw;
    DY[e] = static_cast<float>(p10 - p00 + p11 - p01) * dw;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int region = threadIdx.x >> 2, component = threadIdx.x & 3;
    const int i0 = 5 * (region >> 2), j0 = 5 * (region & 3);
    const float* const src = (component & 1) ? DY : DX;
    float v = 0.f;
    for (int y = i0; y < i0 + 5; ++y)
      for (int x = j0; x < j0 + 5; ++x) {
        const float t = src[y * kPatch + x];
        v = v + (component >= 2 ? fabsf(t) : t);
      }
    vec[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float q = 0.f;
    for (int m = 0; m < 64; ++m) q = q + vec[m] * vec[m];
    scale = 1.f / (sqrtf(q) + static_cast<float>(DBL_EPSILON));
  }
  __syncthreads();
  if (threadIdx.x < 64) descriptors[static_cast<size_t>(blockIdx.x) * 64 + threadIdx.x] = vec[threadIdx.x] * scale;
}

// ---- host ----------------------------------------------------------------------------------------------------------
// the layers of n_octaves x (n_layers + 2) and the floats their arrays take
SurfLayerTable layer_table(int W, int H, int first_octave, int n_octaves, int first_layer, int layers, size_t* floats) {
  SurfLayerTable T = {};
  T.octaves = n_octaves;
  T.layers = layers;
  size_t at = 0;
  for (int o = 0; o < n_octaves; ++o)
    for (int l = 0; l < layers; ++l) {
      SurfLayer& L = T.L[o * layers + l];
      L.size = (DLIOM_SURF_SIZE0 + DLIOM_SURF_SIZE_INCREMENT * (first_layer + l)) << (first_octave + o);
      L.step = 1 << (first_octave + o);
      L.rows = H / L.step;
      L.cols = W / L.step;
      const bool fits = L.size <= H && L.size <= W;
      L.samples_i = fits ? 1 + (H - L.size) / L.step : 0;
      L.samples_j = fits ? 1 + (W - L.size) / L.step : 0;
      L.m = (L.size / 2) / L.step;
      L.offset = static_cast<long long>(at);
      at += static_cast<size_t>(L.rows) * L.cols;
    }
  *floats = at;
  return T;
}

int launch_integral(hipStream_t st, const uint8_t* img, int W, int H, int* S) {
  hipLaunchKernelGGL(surf_row_scan_kernel, dim3(static_cast<unsigned>(H + 1)), dim3(256), 0, st, img, W, S);
  DLIOM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(surf_column_scan_kernel, dim3(blocks_of(W, 256)), dim3(256), 0, st, W, H, S);
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

int launch_layers(hipStream_t st, const int* S, int W, const SurfLayerTable& T, float* det, float* trace) {
  const int entries = T.octaves * T.layers;
  long long most = 0;
  for (int e = 0; e < entries; ++e) most = std::max(most, static_cast<long long>(T.L[e].rows) * T.L[e].cols);
  if (most == 0) return DLIOM_OK;
  hipLaunchKernelGGL(surf_layer_kernel, dim3(blocks_of(most, 256), static_cast<unsigned>(entries)), dim3(256), 0, st, S, W, T, det,
                     trace);
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

int launch_binarize_erode(hipStream_t st, const uint8_t* in, int W, int H, const dliom_surf_options& o, uint8_t* out) {
  hipLaunchKernelGGL(surf_binarize_erode_kernel, dim3(blocks_of(W, kTile), blocks_of(H, kTile)), dim3(256), 0, st, in, W, H,
                     o.binary_threshold, o.structure_element_size, out);
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

int check_image(const void* ctx, const void* image, int32_t width, int32_t height) {
  if (ctx == nullptr || width < 0 || height < 0) return DLIOM_ERR_INVALID_ARGUMENT;
  if (static_cast<int64_t>(width) * height > 0 && image == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  if (static_cast<int64_t>(width) * height > DLIOM_SURF_MAX_PIXELS) return DLIOM_ERR_TOO_LARGE;
  return DLIOM_OK;
}

}  // namespace

int surf_check_options(const dliom_surf_options* o) {
  if (o == nullptr || o->extended != 0 || o->upright != 0 || o->n_octaves < 1 || o->n_octaves > 4 || o->n_octave_layers < 1 ||
      o->n_octave_layers > 3 || !std::isfinite(o->hessian_threshold) || o->hessian_threshold < 0.0 || o->binary_threshold < 0 ||
      o->binary_threshold > 255 || o->structure_element_size < 1 || o->structure_element_size > kMaxK)
    return DLIOM_ERR_INVALID_ARGUMENT;
  return DLIOM_OK;
}

int surf_features_on_device(dliom_ctx* ctx, const uint8_t* image, int W, int H, const dliom_surf_options& o,
                            const float** keypoints, const float** descriptors, int* count) {
  *keypoints = nullptr;
  *descriptors = nullptr;
  *count = 0;
  if (static_cast<int64_t>(W) * H > DLIOM_SURF_MAX_PIXELS) return DLIOM_ERR_TOO_LARGE;
  if (W == 0 || H == 0) return DLIOM_OK;
  hipStream_t st = ctx->stream;
  const size_t pixels = static_cast<size_t>(W) * H;
  size_t layer_floats = 0;
  const SurfLayerTable T = layer_table(W, H, 0, o.n_octaves, 0, o.n_octave_layers + 2, &layer_floats);
  if (T.L[2].samples_i <= 0) return DLIOM_OK;  // not even octave 0's first middle layer has its upper neighbour: no maxima
  // [tables | counters | eroded | S | det | trace | keys | slots | records]
  const size_t o_counters = align256(sizeof(SurfTables)), o_eroded = o_counters + 256, o_S = o_eroded + align256(pixels),
               o_det = o_S + align256(static_cast<size_t>(H + 1) * (W + 1) * 4), o_trace = o_det + align256(layer_floats * 4),
               o_keys = o_trace + align256(layer_floats * 4), o_slots = o_keys + align256(size_t{8} * kMaxKeypoints),
               o_records = o_slots + align256(size_t{4} * kMaxKeypoints),
               total = o_records + align256(size_t{4} * kRecordFloats * kMaxKeypoints);
  const size_t capacity_before = ctx->surf.cap;
  DLIOM_TRY(ctx->surf.reserve(total));
  if (ctx->surf.cap != capacity_before) ctx->surf_tables_ready = false;  // a new allocation: its contents are undefined
  char* const base = ctx->surf.as<char>();
  const SurfTables* const tables = reinterpret_cast<const SurfTables*>(base);
  unsigned* const counters = reinterpret_cast<unsigned*>(base + o_counters);
  uint8_t* const eroded = reinterpret_cast<uint8_t*>(base + o_eroded);
  int* const S = reinterpret_cast<int*>(base + o_S);
  float* const det = reinterpret_cast<float*>(base + o_det);
  float* const trace = reinterpret_cast<float*>(base + o_trace);
  unsigned long long* const keys = reinterpret_cast<unsigned long long*>(base + o_keys);
  unsigned* const slots = reinterpret_cast<unsigned*>(base + o_slots);
  float* const records = reinterpret_cast<float*>(base + o_records);
  if (!ctx->surf_tables_ready) {  // once an allocation of the scratch; the source is a static object
    DLIOM_HIP_TRY(hipMemcpyAsync(base, &kHostTables, sizeof(SurfTables), hipMemcpyHostToDevice, st));
    ctx->surf_tables_ready = true;
  }
  const FillJob clear{counters, 8, 0u};
  DLIOM_TRY(fill_multi(ctx, &clear, 1));
  DLIOM_TRY(launch_binarize_erode(st, image, W, H, o, eroded));
  DLIOM_TRY(launch_integral(st, eroded, W, H, S));
  DLIOM_TRY(launch_layers(st, S, W, T, det, trace));
  {
    long long most = 0;
    for (int oc = 0; oc < o.n_octaves; ++oc) most = std::max(most, static_cast<long long>(T.L[oc * T.layers].rows) * T.L[oc * T.layers].cols);
    hipLaunchKernelGGL(surf_maxima_kernel, dim3(blocks_of(most, 256), static_cast<unsigned>(o.n_octaves * o.n_octave_layers)),
                       dim3(256), 0, st, T, det, trace, static_cast<float>(o.hessian_threshold), counters, keys, slots, records);
    DLIOM_HIP_TRY(hipGetLastError());
  }
  // the two read-backs of a call, each one word through the small read-back region of the page-locked block
  unsigned* const host = pinned_at<unsigned>(ctx, kPinReadback);
  const GatherJob candidates_back{counters, 1};
  DLIOM_TRY(gather_and_wait(ctx, &candidates_back, 1, host));
  const unsigned candidates = host[0];
  if (candidates > static_cast<unsigned>(kMaxKeypoints)) {
    *count = static_cast<int>(std::min<unsigned>(candidates, 0x7fffffffu));
    return DLIOM_ERR_CAPACITY;
  }
  if (candidates == 0) return DLIOM_OK;
  const int n = static_cast<int>(candidates);
  size_t sort_bytes = 0;
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, static_cast<const unsigned long long*>(nullptr),
                                                   static_cast<unsigned long long*>(nullptr), static_cast<const unsigned*>(nullptr),
                                                   static_cast<unsigned*>(nullptr), n, 0, 64, st));
  // [sorted keys | sorted slots | ori | keypoints | frames | descriptors | sort scratch]
  const size_t q_slots = align256(size_t{8} * n), q_ori = q_slots + align256(size_t{4} * n), q_kp = q_ori + align256(size_t{16} * n),
               q_frames = q_kp + align256(size_t{4} * DLIOM_SURF_KEYPOINT_FLOATS * n), q_desc = q_frames + align256(size_t{8} * n),
               q_tmp = q_desc + align256(size_t{4} * DLIOM_SURF_DESCRIPTOR_SIZE * n), total_out = q_tmp + align256(sort_bytes);
  DLIOM_TRY(ctx->surf_out.reserve(total_out));
  char* const ob = ctx->surf_out.as<char>();
  unsigned long long* const sorted_keys = reinterpret_cast<unsigned long long*>(ob);
  unsigned* const sorted_slots = reinterpret_cast<unsigned*>(ob + q_slots);
  float4* const ori = reinterpret_cast<float4*>(ob + q_ori);
  float* const kp = reinterpret_cast<float*>(ob + q_kp);
  float2* const frames = reinterpret_cast<float2*>(ob + q_frames);
  float* const desc = reinterpret_cast<float*>(ob + q_desc);
  DLIOM_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(ob + q_tmp, sort_bytes, keys, sorted_keys, slots, sorted_slots, n, 0, 64, st));
  hipLaunchKernelGGL(surf_orientation_kernel, dim3(static_cast<unsigned>(n)), dim3(64), 0, st, S, W, H, records, sorted_slots, tables,
                     ori);
  DLIOM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(surf_compact_kernel, dim3(1), dim3(64), 0, st, records, sorted_slots, ori, n, kp, frames, counters + 1);
  DLIOM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(surf_descriptor_kernel, dim3(static_cast<unsigned>(n)), dim3(kDescriptorThreads), 0, st, eroded, W, H, kp, frames, counters + 1,
                     tables, desc);
  DLIOM_HIP_TRY(hipGetLastError());
  const GatherJob kept_back{counters + 1, 1};
  DLIOM_TRY(gather_and_wait(ctx, &kept_back, 1, host));  // behind the descriptor kernel: the features are complete
  *keypoints = kp;
  *descriptors = desc;
  *count = static_cast<int>(host[0]);
  return DLIOM_OK;
}

}  // namespace dliom

using namespace dliom;

extern "C" {

dliom_surf_options dliom_surf_default_options(void) {
  dliom_surf_options o;
  o.binary_threshold = 200;
  o.structure_element_size = 3;
  o.hessian_threshold = 400.0;
  o.n_octaves = 4;
  o.n_octave_layers = 3;
  o.extended = 0;
  o.upright = 0;
  return o;
}

int dliom_image_binarize_erode(dliom_ctx* ctx, const uint8_t* image, int32_t width, int32_t height,
                               const dliom_surf_options* options, uint8_t* out) {
  DLIOM_TRY(check_image(ctx, image, width, height));
  DLIOM_TRY(surf_check_options(options));
  const size_t pixels = static_cast<size_t>(width) * height;
  if (pixels == 0) return DLIOM_OK;
  if (out == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(ctx->misc.reserve(2 * align256(pixels)));
  uint8_t* const raw = ctx->misc.as<uint8_t>();
  uint8_t* const eroded = raw + align256(pixels);
  DLIOM_HIP_TRY(hipMemcpyAsync(raw, image, pixels, hipMemcpyHostToDevice, ctx->stream));
  DLIOM_TRY(launch_binarize_erode(ctx->stream, raw, width, height, *options, eroded));
  DLIOM_HIP_TRY(hipMemcpyAsync(out, eroded, pixels, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DLIOM_OK;
}

int dliom_surf_layer(dliom_ctx* ctx, const uint8_t* image, int32_t width, int32_t height, int octave, int layer, float* det,
                     float* trace, int32_t* rows, int32_t* cols) {
  DLIOM_TRY(check_image(ctx, image, width, height));
  if (octave < 0 || octave > 3 || layer < 0 || layer > 4 || rows == nullptr || cols == nullptr || (det == nullptr) != (trace == nullptr))
    return DLIOM_ERR_INVALID_ARGUMENT;
  size_t floats = 0;
  SurfLayerTable T = layer_table(width, height, octave, 1, layer, 1, &floats);
  *rows = T.L[0].rows;
  *cols = T.L[0].cols;
  if (det == nullptr || floats == 0) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  const size_t pixels = static_cast<size_t>(width) * height;
  const size_t o_S = align256(pixels), o_det = o_S + align256(static_cast<size_t>(height + 1) * (width + 1) * 4),
               o_trace = o_det + align256(floats * 4);
  DLIOM_TRY(ctx->misc.reserve(o_trace + align256(floats * 4)));
  char* const base = ctx->misc.as<char>();
  int* const S = reinterpret_cast<int*>(base + o_S);
  DLIOM_HIP_TRY(hipMemcpyAsync(base, image, pixels, hipMemcpyHostToDevice, ctx->stream));
  DLIOM_TRY(launch_integral(ctx->stream, reinterpret_cast<const uint8_t*>(base), width, height, S));
  DLIOM_TRY(launch_layers(ctx->stream, S, width, T, reinterpret_cast<float*>(base + o_det), reinterpret_cast<float*>(base + o_trace)));
  DLIOM_HIP_TRY(hipMemcpyAsync(det, base + o_det, floats * 4, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipMemcpyAsync(trace, base + o_trace, floats * 4, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DLIOM_OK;
}

int dliom_surf_detect_and_compute(dliom_ctx* ctx, const uint8_t* image, int32_t width, int32_t height,
                                  const dliom_surf_options* options, float* keypoints, float* descriptors, int32_t capacity,
                                  int32_t* count) {
  DLIOM_TRY(check_image(ctx, image, width, height));
  DLIOM_TRY(surf_check_options(options));
  if (count == nullptr || capacity < 0 || (keypoints == nullptr) != (descriptors == nullptr)) return DLIOM_ERR_INVALID_ARGUMENT;
  *count = 0;
  const size_t pixels = static_cast<size_t>(width) * height;
  if (pixels == 0) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(ctx->misc.reserve(pixels));
  DLIOM_HIP_TRY(hipMemcpyAsync(ctx->misc.p, image, pixels, hipMemcpyHostToDevice, ctx->stream));
  const float *kp = nullptr, *desc = nullptr;
  int n = 0;
  const int status = surf_features_on_device(ctx, ctx->misc.as<uint8_t>(), width, height, *options, &kp, &desc, &n);
  *count = n;
  if (status != DLIOM_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // the caller's image is consumed on return
    return status;
  }
  if (keypoints == nullptr) {
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DLIOM_OK;
  }
  if (n > capacity) {
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DLIOM_ERR_CAPACITY;
  }
  if (n > 0) {
    DLIOM_HIP_TRY(hipMemcpyAsync(keypoints, kp, static_cast<size_t>(n) * DLIOM_SURF_KEYPOINT_FLOATS * 4, hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipMemcpyAsync(descriptors, desc, static_cast<size_t>(n) * DLIOM_SURF_DESCRIPTOR_SIZE * 4, hipMemcpyDeviceToHost,
                                 ctx->stream));
  }
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DLIOM_OK;
}

}  // extern "C"
