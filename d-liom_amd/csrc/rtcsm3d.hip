// RealTimeCorrelativeScanMatcher3D on gfx950.
//
// Replaces mapping/internal/3d/scan_matching/real_time_correlative_scan_matcher_3d.cc
// (:34-53 Match, :55-95 GenerateExhaustiveSearchTransforms, :97-113 ScoreCandidate).
//
// Pipeline per Match (DESIGN.md "RTCSM3D"):
//   host   window sizes, the (2A+1)^3 candidate rotations normalized(q_init * q_r) and the
//          (2L+1)^3 candidate translations q_init * t_j + t_init, in the reference's float
//          arithmetic (candidate c = j * R + r in generation order z,y,x,rz,ry,rx)
//   GPU A  score volume: exact integer sum_i max(v_i & 0x7fff, 1) per candidate.  run_score_volume
//          starts from the mapping DLIOM_TUNE_SCORE_KERNEL asks for (3 by default) and falls back:
//            3  LDS-box kernel over the grid's dense mirror (score_box.h), when the search suits it:
//               >= 8 translations, >= 2^24 candidate-point pairs, bits <= 7, no refusal of its own
//            2  rotation per lane over the dense mirror (rtcsm_score_dense_kernel): searches the box
//               kernel refuses (W-ref's small ones), and the redo of a match the box kernel flagged
//            1  rotation per lane over the leaf table (rtcsm_score_rot_kernel): grids whose mirror is
//               windowed (bits >= 5) or was not built
//            0  point per lane over the leaf table (rtcsm_score_kernel): bits = 8, whose leaf table
//               needs 64-bit indices
//   GPU B  rigorous float-score interval per candidate from that sum; candidates whose upper
//          bound reaches the best lower bound survive
//   GPU C  survivors only: the reference's SEQUENTIAL float sum in point order, bit-identical
//          (sequential_sums.hip: launch_sequential_sums with the method sequential_sum_method picks
//          for the cloud; dliom_rtcsm3d_sequential_sums runs whichever method its caller names)
//   host   score = sum / N * exp(-(|t| wt + angle wr)^2) as the reference computes it; first
//          strictly greater score in generation order wins.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enums only: the library is resolved at run time (dlopen), see rccl_api()

#include "device_common.h"
#include "host_math.h"
#include "probability_values.h"
#include "rtcsm_bounds.h"
#include "rtcsm_candidates.h"
#include "score_box.h"

namespace dliom {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------------- kernel A
// grid = (point tiles, rotation tiles), 256 threads.  Every thread keeps PPT points of its tile
// in registers (Morton order: the 64 lanes of a wave sit in one small patch of space).  A block
// walks its rotations; for each one it rotates its points once, then walks the T translations
// (uniform -> three scalar loads per translation) and looks up PPT voxels per lane in two
// batches of independent gathers (PPT leaf-table loads, then PPT voxel loads).  The per-lane
// integer sum is reduced across the wave with six DPP adds, combined across the block's four
// waves in LDS, and leaves the block as ONE atomic per candidate per rotation.
// WIDE: 64-bit leaf-table indices, for DynamicGrid bits = 8 ((8 << 8)^3 = 2^33 table entries).
template <int PPT, bool WIDE = false>
__global__ __launch_bounds__(kBlock) void rtcsm_score_kernel(
    GridView g, const float* __restrict__ px, const float* __restrict__ py,
    const float* __restrict__ pz, const float4* __restrict__ rot, int R, int r_first, int r_last,
    const float* __restrict__ trans, int T, int rots_per_block,
    unsigned long long* __restrict__ sums) {
  // Clouds are padded to a multiple of 4096 points with far-away points (kPadCoordinate): those
  // fall outside every grid, read 0 and add exactly 1 each -- the host subtracts the pad count.
  extern __shared__ unsigned block_sum[];  // T entries
  float x[PPT], y[PPT], z[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int i = (blockIdx.x * PPT + k) * kBlock + threadIdx.x;
    x[k] = px[i];
    y[k] = py[i];
    z[k] = pz[i];
  }
  const int r_begin = r_first + blockIdx.y * rots_per_block;  // this shard's rotations only
  const int r_end = min(r_begin + rots_per_block, r_last);
  const int lane = threadIdx.x & 63;
  const float inv = g.inv_resolution;
  typedef typename std::conditional<WIDE, unsigned long long, unsigned>::type idx_t;
  const idx_t sentinel = static_cast<idx_t>(1) << (3 * g.log2_leaves);  // table[L^3] is always 0 (null leaf)
  const unsigned lb = static_cast<unsigned>(g.log2_leaves);
  for (int r = r_begin; r < r_end; ++r) {
    for (int j = threadIdx.x; j < T; j += kBlock) block_sum[j] = 0u;
    __syncthreads();
    const float4 qq = rot[r];
    const Quat4 q{qq.x, qq.y, qq.z, qq.w};  // stored (w,x,y,z)
    float rx[PPT], ry[PPT], rz[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) rotate_point(q, x[k], y[k], z[k], rx[k], ry[k], rz[k]);
#pragma unroll 1
    for (int j = 0; j < T; ++j) {
      const float tx = trans[3 * j], ty = trans[3 * j + 1], tz = trans[3 * j + 2];
      idx_t tix[PPT];
      unsigned cel[PPT];
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const float cx = rx[k] + tx, cy = ry[k] + ty, cz = rz[k] + tz;
        bool near = false;
        int ix = cell_fast(cx, inv, &near);
        int iy = cell_fast(cy, inv, &near);
        int iz = cell_fast(cz, inv, &near);
        if (__builtin_expect(near, 0)) {  // within rounding reach of a cell boundary: exact path
          ix = cell_of(cx, g.resolution);
          iy = cell_of(cy, g.resolution);
          iz = cell_of(cz, g.resolution);
        }
        const unsigned sx = static_cast<unsigned>(ix + g.half);
        const unsigned sy = static_cast<unsigned>(iy + g.half);
        const unsigned sz = static_cast<unsigned>(iz + g.half);
        const bool inside = (sx | sy | sz) < g.grid_size;  // grid_size is a power of two
        const idx_t t = (((static_cast<idx_t>(sz >> 3) << lb) | (sy >> 3)) << lb) | (sx >> 3);
        tix[k] = inside ? t : sentinel;
        cel[k] = ((sz & 7u) << 6) | ((sy & 7u) << 3) | (sx & 7u);
      }
#pragma unroll
      for (int k = 0; k < PPT; ++k) tix[k] = g.table[tix[k]];
#pragma unroll
      for (int k = 0; k < PPT; ++k) cel[k] = g.pool[(static_cast<size_t>(tix[k]) << 9) | cel[k]];
      unsigned a = 0;
#pragma unroll
      for (int k = 0; k < PPT; ++k) a += max(cel[k] & 0x7FFFu, 1u);
      const unsigned total = wave_sum_lane63(a);
      if (lane == 63) atomicAdd(&block_sum[j], total);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < T; j += kBlock)
      atomicAdd(&sums[static_cast<size_t>(j) * R + r], static_cast<unsigned long long>(block_sum[j]));
  }
}

// ---------------------------------------------------------------------------------- kernel A'
// Lanes = candidate ROTATIONS, points are wave-uniform.  grid = (rotation groups of 256, point
// chunks).  Each lane owns one rotation (its quaternion stays in 4 VGPRs) and TC integer
// accumulators, one per translation; the block streams its chunk of points through scalar
// registers (P at a time), rotates each point per lane and looks up the TC translated positions.
// Why: the 64 lanes of a gather now differ only by a few milliradians of rotation of the SAME
// point, so they fall into a handful of neighbouring voxels -- a gather touches ~4 cache lines
// instead of ~40, which removes the texture-addresser bound of the points-per-lane mapping
// (profiles/).  There is no cross-lane reduction at all: a lane's accumulators ARE its
// candidates' partial sums, added to the score volume with 64-lane contiguous atomics.
template <int TC, int P>
__global__ __launch_bounds__(kBlock) void rtcsm_score_rot_kernel(
    GridView g, const float* __restrict__ px, const float* __restrict__ py,
    const float* __restrict__ pz, int points_per_chunk, const float4* __restrict__ rot, int R,
    int r_first, int r_last, const float4* __restrict__ trans4, int T,
    unsigned long long* __restrict__ sums) {
  // LDS: the T translations (read as wave-wide broadcasts) and one accumulator column per lane
  // (TC rows): `lds_acc[jj][lane]` is touched by that lane only -- no conflicts, no barriers.
  extern __shared__ float4 lds_trans[];
  __shared__ unsigned lds_acc[TC][kBlock];
  for (int j = threadIdx.x; j < T; j += kBlock) lds_trans[j] = trans4[j];
  __syncthreads();
  const int r = r_first + blockIdx.x * kBlock + threadIdx.x;
  const bool active = r < r_last;
  const float4 qq = rot[active ? r : r_first];
  const Quat4 q{qq.x, qq.y, qq.z, qq.w};  // stored (w,x,y,z)
  const float inv = g.inv_resolution;
  const unsigned sentinel = 1u << (3 * g.log2_leaves);  // table[L^3] is always 0 (null leaf)
  const unsigned lb = static_cast<unsigned>(g.log2_leaves);
  const int p_begin = blockIdx.y * points_per_chunk;
  const int p_end = p_begin + points_per_chunk;  // the cloud is padded: no tail handling
  for (int jc = 0; jc < T; jc += TC) {
    const int tc = min(TC, T - jc);
    for (int jj = 0; jj < tc; ++jj) lds_acc[jj][threadIdx.x] = 0u;
#pragma unroll 1
    for (int i = p_begin; i < p_end; i += P) {
      float rx[P], ry[P], rz[P];
#pragma unroll
      for (int k = 0; k < P; ++k) rotate_point(q, px[i + k], py[i + k], pz[i + k], rx[k], ry[k], rz[k]);
#pragma unroll 1
      for (int jj = 0; jj < tc; ++jj) {
        const float4 t = lds_trans[jc + jj];  // same address in every lane: LDS broadcast
        unsigned tix[P], cel[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
          const float cx = rx[k] + t.x, cy = ry[k] + t.y, cz = rz[k] + t.z;
          bool near = false;
          int ix = cell_fast(cx, inv, &near);
          int iy = cell_fast(cy, inv, &near);
          int iz = cell_fast(cz, inv, &near);
          if (__builtin_expect(near, 0)) {  // within rounding reach of a cell boundary: exact path
            ix = cell_of(cx, g.resolution);
            iy = cell_of(cy, g.resolution);
            iz = cell_of(cz, g.resolution);
          }
          const unsigned sx = static_cast<unsigned>(ix + g.half);
          const unsigned sy = static_cast<unsigned>(iy + g.half);
          const unsigned sz = static_cast<unsigned>(iz + g.half);
          const bool inside = (sx | sy | sz) < g.grid_size;  // grid_size is a power of two
          const unsigned tt = (((sz >> 3) << lb | (sy >> 3)) << lb) | (sx >> 3);
          tix[k] = inside ? tt : sentinel;
          cel[k] = ((sz & 7u) << 6) | ((sy & 7u) << 3) | (sx & 7u);
        }
#pragma unroll
        for (int k = 0; k < P; ++k) tix[k] = g.table[tix[k]];
#pragma unroll
        for (int k = 0; k < P; ++k) cel[k] = g.pool[(tix[k] << 9) | cel[k]];
        unsigned a = 0;
#pragma unroll
        for (int k = 0; k < P; ++k) a += max(cel[k] & 0x7FFFu, 1u);
        atomicAdd(&lds_acc[jj][threadIdx.x], a);  // ds_add_u32, own column
      }
    }
    if (active) {
      for (int jj = 0; jj < tc; ++jj)
        atomicAdd(&sums[static_cast<size_t>(jc + jj) * R + r],
                  static_cast<unsigned long long>(lds_acc[jj][threadIdx.x]));
    }
  }
}

// ---------------------------------------------------------------------------------- kernel A''
// The same rotation-per-lane walk over the DENSE MIRROR of the grid (grid.hip::ensure_dense):
// one load per lookup, no leaf table, no leaf/cell bit surgery, and the mirror already holds
// max(value, 1), the quantity that is summed.
//   z  = fma(c, 1/res, K)    K = half + 1 + 1/2: shift into the mirror's [0, S) range AND the
//                            half of "floor(x + 1/2)" in the fma's single rounding
//   i' = v_cvt_flr_i32_f32(clamp(z, 0, S - 1/2))   guard cells 0 and S-1 read 1 = "outside/unknown"
//   near <=> some frac(z_c) <= band or >= 1 - band, band = 2.2 S 2^-24 (then: exact path)
//   byte offset = X[ix'] + Y[iy'] + Z[iz']  (LDS tables of the bricked layout, see the kernel)
// Error budget, in cells, with q = c/res the real quotient (|q| <= S/2 inside the grid, z <= S):
//   fl(1/res) relative error 2^-24        -> |c fl(1/res) - q| <= |q| 2^-24     <= (S/2) 2^-24
//   one rounding of the fma               -> <= ulp(z)/2 <= z 2^-24              <=  S    2^-24
//   the reference's lround(fl(q)) can only differ from floor(q + 1/2) when q is within |q| 2^-24
//   of a half-integer (its own rounding of the quotient, and the half-away tie rule)
//                                                                                <= (S/2) 2^-24
// so when z is farther than (2 S + 1) 2^-24 from every integer, floor(z) and the reference agree;
// 2.2 S 2^-24 is used (~6.7e-5 cells at S = 514).  Points far outside the grid break the bounds
// but land in a guard cell on both paths.  The exact path is taken per point (a wave-level branch):
// ~10 % of the 4-point iterations have a near lookup in some lane, usually in one point only.
__device__ __forceinline__ int cvt_flr(float y) {  // floor to int in one instruction
  int r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(y));
  return r;
}

constexpr int kDenseMaxBlock = 256;

// Domain of the per-axis offset tables.  CLAMP = true: [0, S), every lookup is clamped into it
// (v_med3_f32).  CLAMP = false: the host proved that every lookup of this launch -- real points
// within max ||p|| + max |t| of the origin, padding replaced by `pad`, a point that stays beyond the
// grid's edge under every candidate -- lands in [lo, lo + size); entries outside [0, S) alias the
// guard cells, so the three clamps per lookup disappear.
struct DenseDomain {
  int lo;     // mirror coordinate of table entry 0 (<= 0)
  int size;   // entries per axis
  int n_real; // points below this index are real, the rest of the padded arrays is replaced by pad
  float pad[3];
};

template <bool CLAMP>
__global__ __launch_bounds__(kDenseMaxBlock) void rtcsm_score_dense_kernel(
    GridView g, DenseDomain dom, const float* __restrict__ px, const float* __restrict__ py,
    const float* __restrict__ pz, int points_per_chunk, int point_chunks,
    int rot_groups, const float4* __restrict__ rot, int R, int r_first, int r_last,
    const float4* __restrict__ trans4, int T, int t_chunk, unsigned long long* __restrict__ sums) {
  constexpr int P = 8;  // points per iteration (wave-uniform, scalar loads); the host's point chunks are multiples of 8
  // XCD-aware block -> (point chunk, rotation group) map.  Workgroup b lands on XCD b % 8 (observed,
  // used for speed only): the rotation groups of one point chunk run back to back on ONE XCD and
  // share its L2 lines; chunks are dealt to the XCDs round-robin -- giving every XCD one contiguous
  // Morton range of the cloud instead measured 8 % slower (all CUs of an XCD then hammer the few L2
  // channels that hold one compact region of the mirror).
  const int bs = blockDim.x;  // 64..256, picked by the host to waste the fewest lanes on R % bs
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int rot_group = slot % rot_groups;
  const int chunk_id = (slot / rot_groups) * 8 + xcd;
  if (chunk_id >= point_chunks) return;
  extern __shared__ float4 lds_dyn[];  // [T translations | 3 TS byte offsets | t_chunk x blockDim accumulators]
  float4* lds_trans = lds_dyn;
  unsigned* lds_off = reinterpret_cast<unsigned*>(lds_dyn + T);
  const int S = g.dense_stride;
  const int TS = dom.size;  // table entries per axis (S when clamping)
  unsigned* lds_acc = lds_off + 3 * TS;
  for (int j = threadIdx.x; j < T; j += bs) lds_trans[j] = trans4[j];
  // The mirror is stored in 4 x 4 x 4 bricks of 128 B (one cache line): lanes of a wave look up
  // cells a few voxels apart in EVERY direction, and the texture addresser works per distinct line.
  // Per-axis byte offsets come from LDS tables, so the brick swizzle costs no VALU:
  //   offset(x, y, z) = X[x] + Y[y] + Z[z],  X[x] = (x>>2) 128 + (x&3) 2,
  //   Y[y] = (y>>2) B 128 + (y&3) 8,  Z[z] = (z>>2) B^2 128 + (z&3) 32,  B = bricks per axis
  {
    const unsigned B = static_cast<unsigned>(g.dense_bricks);
    for (int c = threadIdx.x; c < TS; c += bs) {
      const unsigned m = static_cast<unsigned>(min(max(c + dom.lo, 0), S - 1));  // outside -> guard cell
      const unsigned h = m >> 2, l = m & 3u;
      lds_off[c] = h * 128u + l * 2u;
      lds_off[TS + c] = h * B * 128u + l * 8u;
      lds_off[2 * TS + c] = h * B * B * 128u + l * 32u;
    }
  }
  __syncthreads();
  const int r = r_first + rot_group * bs + threadIdx.x;
  const bool active = r < r_last;
  const float4 qq = rot[active ? r : r_first];
  const Quat4 q{qq.x, qq.y, qq.z, qq.w};  // stored (w,x,y,z)
  const float inv = g.inv_resolution;
  const float K = static_cast<float>(g.half + 1 - dom.lo) + 0.5f;  // exact: a small integer + 1/2
  const float band = 2.2f * static_cast<float>(TS) * 5.9604645e-8f;
  const float lim = static_cast<float>(TS - 1) + 0.5f;
  const int to_table = g.half + 1 - dom.lo;
  const int p_begin = chunk_id * points_per_chunk;
  const int p_end = p_begin + points_per_chunk;  // the cloud is padded: no tail handling
  // gridDim.y > 1 (small searches): the translation slices are spread over workgroups as well -- a search of a few
  // hundred points fills a fraction of the chip, and each of a workgroup's steps is one exposed gather latency
  for (int jc = blockIdx.y * t_chunk; jc < T; jc += t_chunk * gridDim.y) {
    const int tc = min(t_chunk, T - jc);
    for (int jj = 0; jj < tc; ++jj) lds_acc[jj * bs + threadIdx.x] = 0u;
#pragma unroll 1
    for (int i = p_begin; i < p_end; i += P) {
      float rx[P], ry[P], rz[P];
#pragma unroll
      for (int k = 0; k < P; ++k) {
        // wave-uniform point (scalar loads); without clamps the padding is swapped for dom.pad
        const bool real = CLAMP || i + k < dom.n_real;
        rotate_point(q, real ? px[i + k] : dom.pad[0], real ? py[i + k] : dom.pad[1], real ? pz[i + k] : dom.pad[2],
                     rx[k], ry[k], rz[k]);
      }
#pragma unroll 1
      for (int jj = 0; jj < tc; ++jj) {
        const float4 t = lds_trans[jc + jj];  // same address in every lane: LDS broadcast
        unsigned ox[P], oy[P], oz[P];  // byte offsets of the three clamped mirror coordinates
        float lo[P], hi[P];            // per point: min / max over the axes of frac(z)
#pragma unroll
        for (int k = 0; k < P; ++k) {
          // z = c / res + (half + 1) + 1/2 in ONE rounding; floor(z) is the mirror coordinate
          const float zx = __builtin_fmaf(rx[k] + t.x, inv, K), zy = __builtin_fmaf(ry[k] + t.y, inv, K),
                      zz = __builtin_fmaf(rz[k] + t.z, inv, K);
          const float fx = __builtin_amdgcn_fractf(zx), fy = __builtin_amdgcn_fractf(zy),
                      fz = __builtin_amdgcn_fractf(zz);
          lo[k] = fminf(fminf(fx, fy), fz);
          hi[k] = fmaxf(fmaxf(fx, fy), fz);
          if (CLAMP) {
            // clamp in float (one v_med3_f32): floor(clamp(z, 0, TS - 1/2)) == clamp(floor(z), 0, TS - 1)
            ox[k] = lds_off[cvt_flr(__builtin_amdgcn_fmed3f(zx, 0.f, lim))];
            oy[k] = lds_off[TS + cvt_flr(__builtin_amdgcn_fmed3f(zy, 0.f, lim))];
            oz[k] = lds_off[2 * TS + cvt_flr(__builtin_amdgcn_fmed3f(zz, 0.f, lim))];
          } else {
            ox[k] = lds_off[cvt_flr(zx)];
            oy[k] = lds_off[TS + cvt_flr(zy)];
            oz[k] = lds_off[2 * TS + cvt_flr(zz)];
          }
        }
        float m = lo[0], M = hi[0];
#pragma unroll
        for (int k = 1; k < P; ++k) {
          m = fminf(m, lo[k]);
          M = fmaxf(M, hi[k]);
        }
        if (__builtin_expect(m <= band || M >= 1.f - band, 0)) {
          // some lookup of this lane sits within rounding reach of a cell boundary: the exact
          // division path, but only for the points that need it (one wave-level branch per point)
#pragma unroll
          for (int k = 0; k < P; ++k) {
            if (lo[k] <= band || hi[k] >= 1.f - band) {
              ox[k] = lds_off[min(max(cell_of(rx[k] + t.x, g.resolution) + to_table, 0), TS - 1)];
              oy[k] = lds_off[TS + min(max(cell_of(ry[k] + t.y, g.resolution) + to_table, 0), TS - 1)];
              oz[k] = lds_off[2 * TS + min(max(cell_of(rz[k] + t.z, g.resolution) + to_table, 0), TS - 1)];
            }
          }
        }
        unsigned v[P];
#pragma unroll
        for (int k = 0; k < P; ++k)
          v[k] = *reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(g.dense) + (ox[k] + oy[k] + oz[k]));
        unsigned a = 0;
#pragma unroll
        for (int k = 0; k < P; ++k) a += v[k];  // the mirror stores max(value, 1) already
        atomicAdd(&lds_acc[jj * bs + threadIdx.x], a);  // ds_add_u32, own column
      }
    }
    if (active) {
      for (int jj = 0; jj < tc; ++jj)
        atomicAdd(&sums[static_cast<size_t>(jc + jj) * R + r],
                  static_cast<unsigned long long>(lds_acc[jj * bs + threadIdx.x]));
    }
  }
}

// ---------------------------------------------------------------------------------- kernel B
struct BoundParams {
  double a;        // (double)kScale
  double b;        // (double)(kMin - kScale)
  double delta;    // max |LUT[v] - (a v + b)|, v' convention (0 -> 1)
  double wt, wr;   // penalty weights
  int n;           // points
  int n_pad;       // padding points, each of which added exactly 1 to every sum
  int R, T;
  int r_first, r_last;  // rotations owned by this shard
  SeqSumBoundTable err;  // seq_sum_error_bound(n, U) per binade of U (rtcsm_bounds.h), filled on the host for this n
};

__device__ __forceinline__ float next_up(float f) { return __uint_as_float(__float_as_uint(f) + 1u); }
__device__ __forceinline__ float next_down(float f) {
  const unsigned u = __float_as_uint(f);
  return u == 0u ? 0.f : __uint_as_float(u - 1u);
}

__global__ void rtcsm_bounds_kernel(const unsigned long long* __restrict__ sums, long long C,
                                    const float* __restrict__ t_norm, const float* __restrict__ r_angle,
                                    BoundParams p, float* __restrict__ lo, float* __restrict__ hi,
                                    unsigned* __restrict__ best_lo_bits) {
  const long long c = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool in_range = c < C;
  const int j = in_range ? static_cast<int>(c / p.R) : 0, r = in_range ? static_cast<int>(c % p.R) : 0;
  const bool mine = in_range && r >= p.r_first && r < p.r_last;
  float flo = 0.f, fhi = -1.f;  // another shard's candidate: never a survivor, no lower bound
  if (mine) {
  const double s = static_cast<double>(sums[c] - static_cast<unsigned long long>(p.n_pad));
  const double mid = p.a * s + p.b * p.n;
  const double slack = p.delta * p.n + 1e-9 * mid;
  double sum_lo = mid - slack, sum_hi = mid + slack;
  const double U = sum_hi * (1.0 + 1.0 / 32.0);
  const double e = p.err.err[seq_sum_bound_index(U)];  // = seq_sum_error_bound(p.n, U), which sees U's binade alone
  if (sum_hi + e > U || p.n > (1 << 19)) {  // bound not applicable: keep the candidate
    flo = 0.f;
    fhi = 3.0e38f;
  } else {
    sum_lo -= e;
    sum_hi += e;
    // score = float(double(float(sum)/float(N)) * exp(-(|t| wt + angle wr)^2)); every step is
    // monotone in sum, so outward-rounded endpoints bracket the reference's value.
    const double arg = static_cast<double>(t_norm[j]) * p.wt + static_cast<double>(r_angle[r]) * p.wr;
    const double pen = exp(-(arg * arg));
    const float nf = static_cast<float>(p.n);
    float qlo = next_down(next_down(static_cast<float>(sum_lo))) / nf;
    float qhi = next_up(next_up(static_cast<float>(sum_hi))) / nf;
    qlo = next_down(qlo);
    qhi = next_up(qhi);
    flo = next_down(next_down(static_cast<float>(static_cast<double>(qlo) * pen * (1.0 - 1e-9))));
    fhi = next_up(next_up(static_cast<float>(static_cast<double>(qhi) * pen * (1.0 + 1e-9))));
    if (!(flo > 0.f)) flo = 0.f;
  }
  }
  if (in_range) {
    lo[c] = flo;
    hi[c] = fhi;
  }
  // best lower bound: the wavefront's maximum first (non-negative floats order like their bits), ONE atomic per
  // wavefront -- one per candidate on this one word was most of the kernel (13 us for 35 937 candidates)
  unsigned best = __float_as_uint(flo);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = max(best, static_cast<unsigned>(__shfl_xor(static_cast<int>(best), off, 64)));
  if ((threadIdx.x & 63) == 0 && best != 0u) atomicMax(best_lo_bits, best);
}

__global__ void rtcsm_select_kernel(const float* __restrict__ hi, long long C,
                                    const unsigned* __restrict__ best_lo_bits,
                                    unsigned* __restrict__ count, unsigned* __restrict__ list) {
  const long long c = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float best_lo = __uint_as_float(*best_lo_bits);
  if (hi[c] >= best_lo) {
    const unsigned k = atomicAdd(count, 1u);
    list[k] = static_cast<unsigned>(c);
  }
}

// ---------------------------------------------------------------------------------- probes
__global__ void probe_cells_kernel(Quat4 q, float tx, float ty, float tz, const float* __restrict__ px,
                                   const float* __restrict__ py, const float* __restrict__ pz, int n,
                                   float resolution, int* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float rx, ry, rz;
  rotate_point(q, px[i], py[i], pz[i], rx, ry, rz);
  out[3 * i] = cell_of(rx + tx, resolution);
  out[3 * i + 1] = cell_of(ry + ty, resolution);
  out[3 * i + 2] = cell_of(rz + tz, resolution);
}

// ---------------------------------------------------------------------------------- host side
// Device copies of the candidate tables inside ctx->cand.
struct DeviceCandidates {
  float4* rot;
  float* trans;    // T x 3
  float4* trans4;  // T x (x,y,z,0): 16-byte rows for the rotation-per-lane kernel
  float* t_norm;
  float* r_angle;
  const float4* rot_src;  // where a kernel that runs BEFORE the pending copy (PrepArgs) finds the rotations: the pinned
                          // staging copy while the upload is pending, `rot` itself otherwise
};

// State of a (possibly sharded) match between its phases; lives in dliom_ctx::rtcsm_state.
struct RtcsmState {
  dliom_rtcsm_options o;
  Candidates c;
  DeviceCandidates d;
  dliom_cloud cloud;
  const dliom_grid* grid = nullptr;
  int r_first = 0, r_last = 0;
  unsigned long long* d_sums = nullptr;
  float* d_hi = nullptr;
  unsigned* d_list = nullptr;
  unsigned* d_ctrs = nullptr;
  float best_score = -1.f;
  int64_t best_c = -1;
  bool active = false;
  double init7[7] = {0, 0, 0, 1, 0, 0, 0};
  int shard = 0, num_shards = 1;
  bool used_box = false;
  // host tables that do not fit their page-locked staging region are built here (capacity kept from match to match)
  std::vector<char> host_tables, host_box_tables;
};

static RtcsmState* state_of(dliom_ctx* ctx) {
  if (ctx->rtcsm_state == nullptr) {
    ctx->rtcsm_state = new RtcsmState;
    ctx->rtcsm_state_free = [](void* p) { delete static_cast<RtcsmState*>(p); };
  }
  return static_cast<RtcsmState*>(ctx->rtcsm_state);
}

// ---- pending copies / fills of a match (device_common.h: PrepArgs) --------------------------------------------------
static bool prep_add(PrepArgs* prep, void* dst, const void* src, size_t bytes, unsigned value) {
  if (prep == nullptr || prep->n >= kMaxPrepJobs || (bytes & 3u) != 0 || (reinterpret_cast<uintptr_t>(dst) & 15u) != 0 ||
      (reinterpret_cast<uintptr_t>(src) & 15u) != 0 || bytes / 16 > 0xFFFFFFFFull)
    return false;
  PrepJob& j = prep->job[prep->n++];
  j.dst = static_cast<uint4*>(dst);
  j.src = static_cast<const uint4*>(src);
  j.vec = static_cast<unsigned>(bytes / 16);
  j.tail_words = static_cast<unsigned>((bytes % 16) / 4);
  j.value = value;
  return true;
}
__global__ __launch_bounds__(256) void rtcsm_prep_kernel(PrepArgs a) { prep_block(a, blockIdx.x, gridDim.x, threadIdx.x, blockDim.x); }
// The pending jobs as a launch of their own (score kernels other than the LDS-box one, whose pre-pass carries them).
static int prep_flush(dliom_ctx* ctx, PrepArgs* prep) {
  if (prep == nullptr || prep->n == 0) return DLIOM_OK;
  unsigned most = 1;
  for (int j = 0; j < prep->n; ++j) most = std::max(most, prep->job[j].vec);
  hipLaunchKernelGGL(rtcsm_prep_kernel, dim3(std::min(512u, (most + 255u) / 256u)), dim3(256), 0, ctx->stream, *prep);
  DLIOM_HIP_TRY(hipGetLastError());
  prep->n = 0;
  return DLIOM_OK;
}

// prep != null: the H2D copy becomes a pending job (the staged tables stay in the pinned block until the kernel that
// carries the jobs has run -- every entry point that gets here synchronises the stream before it returns).
static int upload_candidates(dliom_ctx* ctx, const Candidates& c, DeviceCandidates* d, PrepArgs* prep = nullptr) {
  const CandidateTableLayout l = candidate_table_layout(c.num_rotations(), c.trans.size());
  DLIOM_TRY(ctx->cand.reserve(l.total));
  char* base = static_cast<char*>(ctx->cand.p);
  d->rot_src = reinterpret_cast<const float4*>(base);
  if (l.total <= kPinRtcsmCandidates.bytes) {  // (the match's other regions: pinned_layout.h)
    // Pinned staging, written in place: truly asynchronous.
    char* staged = pinned_at<char>(ctx, kPinRtcsmCandidates);
    fill_candidate_tables(c, l, staged);
    if (prep_add(prep, base, staged, l.total, 0u))
      d->rot_src = reinterpret_cast<const float4*>(staged);
    else
      DLIOM_HIP_TRY(hipMemcpyAsync(base, staged, l.total, hipMemcpyHostToDevice, ctx->stream));
  } else {
    std::vector<char>& host = state_of(ctx)->host_tables;
    host.resize(l.total);
    fill_candidate_tables(c, l, host.data());
    DLIOM_HIP_TRY(hipMemcpyAsync(base, host.data(), l.total, hipMemcpyHostToDevice, ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // `host` is the next match's as well
  }
  d->rot = reinterpret_cast<float4*>(base + l.rot);
  d->trans = reinterpret_cast<float*>(base + l.trans);
  d->t_norm = reinterpret_cast<float*>(base + l.t_norm);
  d->r_angle = reinterpret_cast<float*>(base + l.r_angle);
  d->trans4 = reinterpret_cast<float4*>(base + l.trans4);
  return DLIOM_OK;
}

static int env_int(const char* name, int fallback) { return tuning_int(name, fallback); }  // experiments builds only

#ifdef DLIOM_EXPERIMENTS
// Host time of a match from match_begin()'s entry to its first launch, and to the laps on the way (DLIOM_HOST_PREP_TIMING=1:
// one line on stderr when the library is unloaded; tools/critical_path.py reads it).  Laps: 0 candidates generated,
// 1 tables staged, 2 mirror and Morton copies ensured, 3 box tables built, 4 span opened, 5 = the total.
struct HostPrepClock {
  static constexpr int kLaps = 6;
  std::chrono::steady_clock::time_point t0;
  std::vector<float> us[kLaps];
  void start() { t0 = std::chrono::steady_clock::now(); }
  void lap(int k) { us[k].push_back(std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - t0).count()); }
  void stop() { lap(kLaps - 1); }
  ~HostPrepClock() {
    std::vector<float>& total = us[kLaps - 1];
    if (total.empty() || env_int("DLIOM_HOST_PREP_TIMING", 0) == 0) return;
    double sum = 0.0;
    for (float v : total) sum += v;
    for (std::vector<float>& v : us) std::sort(v.begin(), v.end());
    std::fprintf(stderr, "rtcsm host prep: matches %zu mean_us %.2f median_us %.2f min_us %.2f lap_medians_us", total.size(),
                 sum / total.size(), total[total.size() / 2], total.front());
    for (const std::vector<float>& v : us) std::fprintf(stderr, " %.2f", v.empty() ? 0.f : v[v.size() / 2]);
    std::fprintf(stderr, "\n");
  }
};
static HostPrepClock g_host_prep;
#define DLIOM_PREP_LAP(k) g_host_prep.lap(k)
#else
#define DLIOM_PREP_LAP(k) ((void)0)
#endif

// LDS-box score kernel (score_box.h): builds the per-pass constants in double and launches it.
// Returns DLIOM_ERR_CAPACITY when the search does not suit the kernel (the caller then uses the dense
// kernel): boxes that cannot hold a typical point's lookups, or coordinates beyond the scaled range.
static int launch_score_box(dliom_ctx* ctx, const dliom_cloud& cloud, const GridView& g, const Candidates& c,
                            const DeviceCandidates& d, int r_first, int r_last, unsigned long long* d_sums,
                            unsigned* d_error, PrepArgs* prep) {
  using namespace box;
  const int R = static_cast<int>(c.w.num_rotations), T = static_cast<int>(c.w.num_translations);
  const int n = static_cast<int>(cloud.n);
  // Which instantiation (score_box.h; round 6, A/B on BASELINE configs 2 and 5 in one process each):
  //   0  27 translations per pass, four waves per SIMD, 14 336-cell boxes: a window of ONE pass (config 2: 0.69 ms; the
  //      same kernel at three waves per SIMD 0.71, with 21 000-cell boxes 0.70, with 64-point chunks 0.70-0.72)
  //   1  the same at three waves per SIMD (168 registers) with 21 000-cell boxes: windows of several passes, whose
  //      translations reach further and make the boxes larger (config 5: 221 -> 195 ms)
  //   2  49 translations per pass at three waves per SIMD, 21 000-cell boxes: one staged box and one rotation per point
  //      serve 49 translations (a whole z-plane of config 5's 7^3 window: 159 ms; with 54 per pass 180) -- where its
  //      padding costs less than the 13 % of vector instructions per lookup it saves, by a margin (the wide kernel is
  //      measured at 343 translations only)
  static const int forced_variant = env_int("DLIOM_BOX_VARIANT", -1);
  const auto padded = [T](int tc) { return ((T + tc - 1) / tc) * tc; };
  const int variant = forced_variant >= 0 && forced_variant <= 2
                          ? forced_variant
                          : (T <= kTC ? 0 : (0.87 * padded(kTCWide) < 0.9 * padded(kTC) ? 2 : 1));
  const int TC = variant == 2 ? kTCWide : kTC;
  static const int forced_cells = env_int("DLIOM_BOX_CELLS", 0);
  const int cells = forced_cells > 0 ? forced_cells : (variant == 0 ? 14336 : 21000);
  // 64-point chunks where the boxes are large (config 5, same runs: 195 -> 189 ms at 27 translations per pass, 187 -> 181
  // at 54); on config 2's narrow kernel they cost 1-3 % (0.70-0.72 against 0.69 ms)
  static const int forced_chunk = env_int("DLIOM_BOX_CHUNK", 0);
  const int chunk_pts = forced_chunk > 0 ? forced_chunk : (variant == 0 ? kCostChunk : kCostChunkBig);
  const double res = static_cast<double>(g.resolution);
  const int passes = (T + TC - 1) / TC;
  // ---- error budget (score_box.h): E / u = 1 + (2 qmax + rmax + taumax) / 256
  double tmax = 0.0;
  for (const F3& t : c.trans) tmax = std::max(tmax, static_cast<double>(std::max(std::fabs(t.x), std::max(std::fabs(t.y), std::fabs(t.z)))));
  const double rmax = static_cast<double>(cloud.max_norm) / res + 1.0;
  const double qmax = rmax + tmax / res + 1.0;
  // Two different limits (round 5 separated them; until then the absolute coordinate was held below 880 cells, i.e. the
  // kernel only ran within 88 m of a 10 cm grid's origin): (i) Kb = (gi - lo) + f must be exact in a float with its 14
  // fraction bits, |gi - lo| < 1024 -- gi is the pass's translation and lo the box's origin, both ABSOLUTE cell
  // coordinates, and their difference is 128 minus the rotated point's cell: a limit on the scan's RANGE (checked below
  // with taumax, and per box in the kernel); (ii) the absolute coordinate q = (r + t) / res enters only the error budget
  // (the reference's own float rounding of r + t and of the quotient, 2 |q| 2^-24): the band widens with it, nothing
  // breaks -- any cell DynamicGrid can address (|q| < 8192 + range) is fine.
  if (!std::isfinite(qmax) || qmax > 16500.0) return (ctx->last_box_refusal = DLIOM_BOX_REFUSED_RANGE, DLIOM_ERR_CAPACITY);
  // ---- waves per workgroup, rotation blocks (what the tables' sizes depend on)
  const int rot_groups_all = (r_last - r_first + 63) / 64;
  static const int forced_nw = env_int("DLIOM_BOX_NW", 0);  // tuning knob
  const int nw = forced_nw >= 1 && forced_nw <= kWaves
                     ? std::min(forced_nw, rot_groups_all)
                     : std::min(rot_groups_all, kWaves);  // four waves = one per SIMD: measured 2-3 % faster than three even
                                                          // when that leaves idle waves in the last rotation block
  const int rot_blocks = (rot_groups_all + nw - 1) / nw;
  // ---- host tables [tau | passes | groups | bitmaps], built where they are staged: in the pinned block when they fit
  // (a few KB), else in the match state's own buffer.  A refusal below leaves them half written: nobody reads them then.
  const size_t tau_count = static_cast<size_t>(passes) * TC * 4, bitmap_count = static_cast<size_t>(passes) * kBitmapWords;
  const size_t tau_bytes = align256(tau_count * 4);
  const size_t pass_only_bytes = align256(static_cast<size_t>(passes) * sizeof(Pass));
  const size_t group_bytes = align256(static_cast<size_t>(rot_blocks) * sizeof(Group));
  const size_t bitmap_bytes = align256(bitmap_count * 4);
  const size_t pass_bytes = pass_only_bytes + group_bytes + bitmap_bytes;  // [passes | groups | bitmaps]
  const bool tables_staged = tau_bytes + pass_bytes <= kPinBoxTables.bytes;
  char* h = nullptr;
  if (tables_staged) {
    h = pinned_at<char>(ctx, kPinBoxTables);
  } else {
    std::vector<char>& host = state_of(ctx)->host_box_tables;
    host.resize(tau_bytes + pass_bytes);
    h = host.data();
  }
  float* const tau = reinterpret_cast<float*>(h);
  Pass* const pass = reinterpret_cast<Pass*>(h + tau_bytes);
  unsigned* const bitmap = reinterpret_cast<unsigned*>(h + tau_bytes + pass_only_bytes + group_bytes);
  std::memset(tau, 0, tau_count * 4);
  std::memset(pass, 0, static_cast<size_t>(passes) * sizeof(Pass));
  double taumax = 0.0;
  for (int tp = 0; tp < passes; ++tp) {  // pass centres first: taumax enters the band
    const int j0 = tp * TC, tc = std::min(TC, T - j0);
    for (int a = 0; a < 3; ++a) {
      double lo = 1e300, hi = -1e300;
      for (int j = j0; j < j0 + tc; ++j) {
        const double v = a == 0 ? c.trans[j].x : (a == 1 ? c.trans[j].y : c.trans[j].z);
        lo = std::min(lo, v);
        hi = std::max(hi, v);
      }
      taumax = std::max(taumax, (hi - lo) * 0.5 / res + 1.0);
    }
  }
  if (rmax + taumax + 130.0 > 1000.0) return (ctx->last_box_refusal = DLIOM_BOX_REFUSED_RANGE, DLIOM_ERR_CAPACITY);  // (i)
  const double e16 = 1.0 + (2.0 * qmax + rmax + taumax) / 256.0;
  const int B = static_cast<int>(std::ceil(e16 + 0.25));
  const int s_units = B;
  const double u = 1.0 / 65536.0;
  for (int tp = 0; tp < passes; ++tp) {
    Pass& ps = pass[static_cast<size_t>(tp)];
    ps.j0 = tp * TC;
    ps.tc = std::min(TC, T - ps.j0);
    ps.pad[0] = ps.pad[1] = 0;
    for (int a = 0; a < 3; ++a) {
      auto comp = [&](int j) { return static_cast<double>(a == 0 ? c.trans[j].x : (a == 1 ? c.trans[j].y : c.trans[j].z)); };
      double lo = 1e300, hi = -1e300;
      for (int j = ps.j0; j < ps.j0 + ps.tc; ++j) {
        lo = std::min(lo, comp(j));
        hi = std::max(hi, comp(j));
      }
      const double tcen = 0.5 * (lo + hi);
      const double G = tcen / res + 128.5 + s_units * u;
      const double gi = std::floor(G);
      const double f = std::nearbyint((G - gi) * 16384.0) / 16384.0;  // 14 fractional bits (may be 1.0)
      ps.gi[a] = static_cast<int>(gi);
      ps.f[a] = static_cast<float>(f);
      ps.uc[a] = static_cast<float>(tcen / res + 0.5);
      double reach = 0.0;
      for (int jj = 0; jj < TC; ++jj) {
        const int j = ps.j0 + std::min(jj, ps.tc - 1);  // short pass: padding repeats the last translation
        const double tv = comp(j) / res + 128.5 + s_units * u - (gi + f);
        const float tf = static_cast<float>(tv);
        tau[(static_cast<size_t>(tp) * TC + jj) * 4 + a] = tf;
        reach = std::max(reach, std::fabs(static_cast<double>(tf)));
      }
      // + the float roundings of the bounding box's own arithmetic at this distance from the origin (interval end +
      // pass centre: values up to qmax, four roundings of half an ulp each; 0.0002 of the kernel's slack covers < 1024)
      ps.reach[a] = static_cast<float>(reach + 0.02 + qmax * std::ldexp(1.0, -22));
    }
  }
  // ---- band bitmap: fractions phi of a scaled coordinate for which SOME translation of the pass gives
  // frac16(fl(phi + tau_j)) <= thr, i.e. frac(phi + tau_j) in [-u/2, (thr + 1/2) u]; one u of margin each side
  std::memset(bitmap, 0, bitmap_count * 4);
  const unsigned thr_units = static_cast<unsigned>(s_units + B);
  for (int tp = 0; tp < passes; ++tp) {
    const Pass& ps = pass[static_cast<size_t>(tp)];
    for (int a = 0; a < 3; ++a) {
      unsigned* words = bitmap + static_cast<size_t>(tp) * kBitmapWords + static_cast<size_t>(a) * (kBuckets / 32);
      for (int jj = 0; jj < ps.tc; ++jj) {
        const double tv = static_cast<double>(tau[(static_cast<size_t>(tp) * TC + jj) * 4 + a]);
        const double af = tv - std::floor(tv);
        const double L = -af - 1.5 * u, H = -af + (thr_units + 1.5) * u;
        const long long b0 = static_cast<long long>(std::floor(L * kBuckets)), b1 = static_cast<long long>(std::floor(H * kBuckets));
        for (long long b = b0; b <= b1; ++b) {
          const unsigned m = static_cast<unsigned>(((b % kBuckets) + kBuckets) % kBuckets);
          words[m >> 5] |= 1u << (m & 31u);
        }
      }
    }
  }
  // ---- does a typical point fit?  spread of one point over 64 consecutive rotations <= 2 * 11 steps * rho
  {
    const double step = c.w.angular_step_size;
    const double a_lanes = (2.0 * c.w.angular_window_size + 1.0) * step;  // rotation-vector span of a workgroup (per axis, at most)
    const double spread = a_lanes * 0.6 * cloud.max_norm / res;                        // cells, at 60 % of the maximum range
    const double dim = spread + 2.0 * taumax + 8.0;
    if (dim > kMaxDim || dim * dim * (dim * 0.25) > cells) return (ctx->last_box_refusal = DLIOM_BOX_REFUSED_WINDOW, DLIOM_ERR_CAPACITY);
  }
  // ---- spread of every wave's 64 rotations around its centre lane (window only: q_init cancels)
  if (TC * sizeof(float4) + kBitmapWords * 4 + 16 + static_cast<size_t>(nw) * kListWords * 4 + static_cast<size_t>(cells) * 2 >
      160 * 1024)
    return (ctx->last_box_refusal = DLIOM_BOX_REFUSED_LDS, DLIOM_ERR_CAPACITY);  // LDS budget (checked again where the launch is sized)
  struct GroupCache {  // depends on the window and the shard only: cached per thread across matches
    int A = -1, r_first = -1, r_last = -1, nw = 0;
    float step = 0.f;
    std::vector<Group> groups;
  };
  static thread_local GroupCache gcache;
  const bool gcache_hit = gcache.A == c.w.angular_window_size && gcache.step == c.w.angular_step_size &&
                          gcache.r_first == r_first && gcache.r_last == r_last && gcache.nw == nw;
  std::vector<Group>& groups = gcache.groups;
  if (!gcache_hit) {
    gcache.A = -1;
    groups.assign(static_cast<size_t>(rot_blocks), Group());
  }
  for (size_t gi = 0; !gcache_hit && gi < groups.size(); ++gi) {
    Group& gr = groups[gi];
    const int r0 = r_first + static_cast<int>(gi) * nw * 64;
    const int cnt = std::max(0, std::min(nw * 64, r_last - r0));
    gr.c_lane = cnt / 2;
    gr.theta2 = 0.f;
    for (int a = 0; a < 3; ++a) gr.dc[a] = gr.hd[a] = 0.f;
    if (cnt <= 0) {
      gr.c_lane = 0;
      continue;
    }
    RotationSpread sp;  // of the block's rotations around its centre lane (rtcsm_candidates.h)
    rotation_spread(c, r0, cnt, &sp);
    const double th = sp.max_angle;
    if (th > 0.3) return (ctx->last_box_refusal = DLIOM_BOX_REFUSED_WINDOW, DLIOM_ERR_CAPACITY);  // the second-order bound below assumes small relative rotations
    for (int a = 0; a < 3; ++a) {
      gr.dc[a] = static_cast<float>(0.5 * (sp.lo[a] + sp.hi[a]));
      gr.hd[a] = static_cast<float>(0.5 * (sp.hi[a] - sp.lo[a]) * 1.0001 + 1e-7);
    }
    gr.theta2 = static_cast<float>(0.51 * th * th * 1.01 + 1e-9);
  }
  gcache.A = c.w.angular_window_size;
  gcache.step = c.w.angular_step_size;
  gcache.r_first = r_first;
  gcache.r_last = r_last;
  gcache.nw = nw;
  DLIOM_PREP_LAP(3);
  // every refusal (DLIOM_ERR_CAPACITY) is behind us: the launch below is what DLIOM_KERNEL_RTCSM_SCORE times
  struct SpanGuard {
    dliom_ctx* c;
    int span;
    ~SpanGuard() { c->end_span(span); }
  } span_guard{ctx, ctx->begin_span(DLIOM_KERNEL_RTCSM_SCORE)};
  DLIOM_PREP_LAP(4);
  // ---- device tables (after the candidate tables inside ctx->cand would alias uploads in flight: own buffer)
  DLIOM_TRY(ctx->box_tables.reserve(tau_bytes + pass_bytes));
  char* base = static_cast<char*>(ctx->box_tables.p);
  const Group* group_src = reinterpret_cast<const Group*>(base + tau_bytes + pass_only_bytes);  // for the pre-pass (below)
  std::memcpy(h + tau_bytes + pass_only_bytes, groups.data(), groups.size() * sizeof(Group));
  if (tables_staged) {
    if (prep_add(prep, base, h, tau_bytes + pass_bytes, 0u))  // rides in the pre-pass, which reads its groups from the staging copy
      group_src = reinterpret_cast<const Group*>(h + tau_bytes + pass_only_bytes);
    else
      DLIOM_HIP_TRY(hipMemcpyAsync(base, h, tau_bytes + pass_bytes, hipMemcpyHostToDevice, ctx->stream));
  } else {
    DLIOM_HIP_TRY(hipMemcpyAsync(base, h, tau_bytes + pass_bytes, hipMemcpyHostToDevice, ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // pageable: the buffer is the next match's as well
  }
  Params p;
  p.tau = reinterpret_cast<const float4*>(base);
  p.pass = reinterpret_cast<const Pass*>(base + tau_bytes);
  p.group = reinterpret_cast<const Group*>(base + tau_bytes + pass_only_bytes);
  p.bitmap = reinterpret_cast<const unsigned*>(base + tau_bytes + pass_only_bytes + group_bytes);
  p.trans = d.trans;
  p.rot = d.rot;
  p.sums = d_sums;
  p.error = d_error;
  p.R = R;
  p.r_first = r_first;
  p.r_last = r_last;
  p.T = T;
  p.passes = passes;
  p.n = n;
  p.chunk = std::min(kMaxChunk, std::max(4, chunk_pts & ~3));
  p.order = p.chunk == kCostChunk ? cloud.d_chunk_order : (p.chunk == kCostChunkBig ? cloud.d_chunk_order_big : nullptr);
  p.point_chunks = (n + p.chunk - 1) / p.chunk;
  const int rot_groups = (r_last - r_first + 63) / 64;
  p.rot_groups = rot_groups;
  p.rot_blocks = rot_blocks;
  p.nw = nw;
  p.thr = thr_units;
  p.cells = cells;
  static const int split_points = env_int("DLIOM_BOX_SPLIT", 1);  // experiments builds: 0 = idle waves in a short rotation block
  p.split_points = split_points;
#ifdef DLIOM_EXPERIMENTS
  static const int box_debug = env_int("DLIOM_BOX_DEBUG", 0);
  p.debug = box_debug;
  if (box_debug & 512) p.order = nullptr;
#else
  p.debug = 0;
#endif
  const size_t lds = TC * sizeof(float4) + kBitmapWords * 4 + 16 + static_cast<size_t>(nw) * kListWords * 4 +
                     static_cast<size_t>(cells) * 2;
  if (lds > 160 * 1024) return (ctx->last_box_refusal = DLIOM_BOX_REFUSED_LDS, DLIOM_ERR_CAPACITY);
  typedef void (*BoxKernel)(GridView, Params, const float*, const float*, const float*);
  const BoxKernel kernel = variant == 0 ? rtcsm_score_box_kernel : (variant == 1 ? rtcsm_score_box_kernel_w3 : rtcsm_score_box_kernel_wide);
  const unsigned attr_bit = variant == 0 ? kFuncAttrScoreBox : (variant == 1 ? kFuncAttrScoreBoxW3 : kFuncAttrScoreBoxWide);
  if ((ctx->func_attr_set & attr_bit) == 0u) {
    DLIOM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ctx->func_attr_set |= attr_bit;
  }
  ctx->last_box_variant = variant;
  // workgroups: one round of residents (every wave walks an equal share of the point chunks, so a second,
  // partly filled round would only idle)
  static thread_local size_t resident_lds = 0;
  static thread_local int resident = 0, resident_nw = 0, resident_variant = -1;
  if (resident_lds != lds || resident_nw != nw || resident_variant != variant) {
    resident_nw = nw;
    resident_variant = variant;
    DLIOM_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, reinterpret_cast<const void*>(kernel), 64 * nw, lds));
    resident_lds = lds;
  }
  const int want_blocks = std::max(1, resident) * ctx->num_cus;
  int slot_quads = std::max(1, want_blocks / std::max(1, rot_blocks * passes));
  slot_quads = std::min(slot_quads, p.point_chunks);
  // (32-bit register accumulators: the kernel adds them to the 64-bit volume every box::kFlushPoints points)
  p.slots = slot_quads;
  p.units = passes * rot_blocks;
  DLIOM_TRY(ctx->box_counters.reserve(static_cast<size_t>(passes) * rot_blocks * 4 + 256));
  if (!prep_add(prep, ctx->box_counters.p, nullptr, static_cast<size_t>(passes) * rot_blocks * 4, 0u))
    DLIOM_HIP_TRY(hipMemsetAsync(ctx->box_counters.p, 0, static_cast<size_t>(passes) * rot_blocks * 4, ctx->stream));
  p.counters = ctx->box_counters.as<unsigned>();
  // per-(rotation block, point) extents of the lookups: the boxes' bounding boxes are reductions over these
  p.ext_stride = static_cast<int>(cloud.n_padded);
  DLIOM_TRY(ctx->box_extents.reserve(static_cast<size_t>(rot_blocks) * 6 * static_cast<size_t>(cloud.n_padded) * 4));
  p.ext = ctx->box_extents.as<float>();
#ifdef DLIOM_EXPERIMENTS
  g_host_prep.stop();
#endif
  {
    // the pre-pass is the first kernel of the match: one more row of workgroups carries the pending copies and fills
    PrepArgs none;
    none.n = 0;
    const PrepArgs& jobs = prep != nullptr ? *prep : none;
    const unsigned prep_rows = jobs.n > 0 ? 1u : 0u;
    hipLaunchKernelGGL(rtcsm_box_extent_kernel, dim3(static_cast<unsigned>((n + 255) / 256), static_cast<unsigned>(rot_blocks) + prep_rows),
                       dim3(256), 0, ctx->stream, p, g.inv_resolution, cloud.d_xs, cloud.d_ys, cloud.d_zs, ctx->box_extents.as<float>(),
                       group_src, d.rot_src, jobs);
    if (prep != nullptr) prep->n = 0;
  }
  const unsigned blocks = static_cast<unsigned>(slot_quads) * passes * rot_blocks;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * nw), lds, ctx->stream, g, p, cloud.d_xs, cloud.d_ys, cloud.d_zs);
  DLIOM_HIP_TRY(hipGetLastError());
#ifdef DLIOM_TEST_HOOKS  // libdliom_hooks.so only (make hooks): as if the kernel had flagged an inconsistency
  if (ctx->tuning[DLIOM_TUNE_RESERVED_TEST_HOOK] == 1) {  // 1 only: 2 and 3 are the de-skew check's hooks (preprocess.hip)
    ctx->tuning[DLIOM_TUNE_RESERVED_TEST_HOOK] = 0;
    DLIOM_HIP_TRY(hipMemsetAsync(static_cast<char*>(ctx->box_error.p) + 4, 1, 1, ctx->stream));
  }
#endif
  return DLIOM_OK;
}

// The fallback score kernels below: point chunks are halved until a launch has at least this many workgroups.
constexpr int kScoreTargetBlocks = 8192;

// Mapping 2: rotation per lane over the dense mirror (rtcsm_score_dense_kernel).  *processed = points visited, padding
// included.
static int launch_score_dense(dliom_ctx* ctx, const dliom_cloud& cloud, const GridView& g, const Candidates& c,
                              const DeviceCandidates& d, int r_first, int r_last, unsigned long long* d_sums,
                              int64_t* processed) {
  const int R = static_cast<int>(c.w.num_rotations), T = static_cast<int>(c.w.num_translations);
  const int n = static_cast<int>(cloud.n);
  const int Rs = r_last - r_first;  // rotations of this shard
  const size_t trans_lds = static_cast<size_t>(T) * 16;
  if (trans_lds > 100 * 1024) return DLIOM_ERR_INVALID_ARGUMENT;
  // block size: whole wavefronts, the fewest idle lanes in the last rotation group
  int bs = kDenseMaxBlock;
  for (int cand = kDenseMaxBlock; cand >= 64; cand -= 64)
    if ((Rs + cand - 1) / cand * cand < (Rs + bs - 1) / bs * bs) bs = cand;
  // small searches (a few hundred points after the adaptive voxel filter) would fill a handful
  // of workgroups: go down to one wavefront per group and 8-point chunks to spread them
  if (static_cast<int64_t>((Rs + bs - 1) / bs) * ((n + 63) / 64) < 256) bs = 64;
  const int rot_groups = (Rs + bs - 1) / bs;
  int chunk = 4096;
  while (chunk > 8 && static_cast<int64_t>(rot_groups) * ((n + chunk - 1) / chunk) < kScoreTargetBlocks) chunk >>= 1;
  const int point_chunks = (n + chunk - 1) / chunk;
  *processed = static_cast<int64_t>(point_chunks) * chunk;
  // Table domain: all real lookups lie within max ||p|| + max |translation component| of the origin.
  DenseDomain dom;
  dom.lo = 0;
  dom.size = g.dense_stride;
  dom.n_real = n;
  dom.pad[0] = dom.pad[1] = dom.pad[2] = kPadCoordinate;
  bool clamp = true;
  {
    float tmax = 0.f, t_init = norm3(c.init.t);
    for (const F3& t : c.trans) tmax = std::max(tmax, std::max(std::fabs(t.x), std::max(std::fabs(t.y), std::fabs(t.z))));
    const float res = g.resolution;
    const double reach = (static_cast<double>(cloud.max_norm) + tmax) / res + 3.0;  // cells from the origin
    // padding point: W = ((half + m) res, 0, 0) in the grid frame, mapped back through the initial
    // pose; under a candidate it moves by at most theta_max |W - t_init| + (L + 1) res sqrt(3)
    const double theta_max = 1.7321 * (c.w.angular_window_size + 1) * c.w.angular_step_size * 1.01 + 1e-4;
    const double rho = (g.half + 64) * static_cast<double>(res) + t_init;
    const double m_cells = 8.0 + std::ceil((theta_max * rho + (c.w.linear_window_size + 1) * res * 1.7321) / res);
    // the padding point itself may be carried up to (m - 8) cells outward as well
    const double hi_cell = std::max(reach, g.half + 2.0 * m_cells);
    const int lo_i = std::min(0, g.half + 1 - static_cast<int>(std::ceil(hi_cell)));
    const int hi_i = std::max(g.dense_stride, g.half + 1 + static_cast<int>(std::ceil(hi_cell)) + 1);
    if (m_cells <= 64.0 && hi_i - lo_i <= 1024 && std::isfinite(reach)) {
      clamp = false;
      dom.lo = lo_i;
      dom.size = hi_i - lo_i;
      const F3 w{static_cast<float>((g.half + m_cells) * res) - c.init.t.x, -c.init.t.y, -c.init.t.z};
      const QF qi{c.init.q.w, -c.init.q.x, -c.init.q.y, -c.init.q.z};
      const F3 p = qrot(qi, w);
      dom.pad[0] = p.x;
      dom.pad[1] = p.y;
      dom.pad[2] = p.z;
    }
  }
  // translations per pass over the points: up to 27, as many as keep >= 4 workgroups per CU in LDS (160 KB);
  // large windows / big grids trade a few extra point rotations for occupancy
  const size_t fixed_lds = trans_lds + static_cast<size_t>(dom.size) * 12;
  const size_t acc_budget = fixed_lds < 34 * 1024 ? 36 * 1024 - fixed_lds : 2 * 1024;
  int t_chunk = std::max(4, std::min(std::min(T, 27), static_cast<int>(acc_budget / (static_cast<size_t>(bs) * 4))));
  const int chunks_per_xcd = (point_chunks + 7) / 8;
  // small searches (the reference's ~170 filtered points): translation slices over gridDim.y until ~4 workgroups per CU
  int t_slices = 1;
  const int base_blocks = 8 * chunks_per_xcd * rot_groups;
  if (base_blocks < 512 && T > 1) {
    const int want = std::min(T, (1024 + base_blocks - 1) / base_blocks);
    t_chunk = std::min(t_chunk, (T + want - 1) / want);
    t_slices = (T + t_chunk - 1) / t_chunk;
  }
  const size_t lds = fixed_lds + static_cast<size_t>(t_chunk) * bs * 4;
  const auto kernel = clamp ? &rtcsm_score_dense_kernel<true> : &rtcsm_score_dense_kernel<false>;
  const int span = ctx->begin_span(DLIOM_KERNEL_RTCSM_SCORE);
  hipLaunchKernelGGL(kernel, dim3(base_blocks, t_slices), dim3(bs), lds, ctx->stream, g, dom, cloud.d_xs, cloud.d_ys,
                     cloud.d_zs, chunk, point_chunks, rot_groups, d.rot, R, r_first, r_last, d.trans4, T, t_chunk, d_sums);
  ctx->end_span(span);
  return DLIOM_OK;
}

// Mapping 1: rotation per lane over the leaf table (rtcsm_score_rot_kernel).  *processed as above.
static int launch_score_rot(dliom_ctx* ctx, const dliom_cloud& cloud, const GridView& g, const Candidates& c,
                            const DeviceCandidates& d, int r_first, int r_last, unsigned long long* d_sums,
                            int64_t* processed) {
  const int R = static_cast<int>(c.w.num_rotations), T = static_cast<int>(c.w.num_translations);
  const int n = static_cast<int>(cloud.n);
  const size_t lds = static_cast<size_t>(T) * 16;
  if (lds > 100 * 1024) return DLIOM_ERR_INVALID_ARGUMENT;
  const int rot_groups = (r_last - r_first + kBlock - 1) / kBlock;
  // points per chunk: a power of two dividing the 4096-point padding
  int chunk = 4096;
  while (chunk > 64 && static_cast<int64_t>(rot_groups) * ((n + chunk - 1) / chunk) < kScoreTargetBlocks) chunk >>= 1;
  const int point_chunks = (n + chunk - 1) / chunk;
  *processed = static_cast<int64_t>(point_chunks) * chunk;
  const auto kernel = T == 1 ? &rtcsm_score_rot_kernel<1, 4> : &rtcsm_score_rot_kernel<27, 8>;
  const int span = ctx->begin_span(DLIOM_KERNEL_RTCSM_SCORE);
  hipLaunchKernelGGL(kernel, dim3(rot_groups, point_chunks), dim3(kBlock), lds, ctx->stream, g, cloud.d_xs, cloud.d_ys,
                     cloud.d_zs, chunk, d.rot, R, r_first, r_last, d.trans4, T, d_sums);
  ctx->end_span(span);
  return DLIOM_OK;
}

// Mapping 0: point per lane over the leaf table (rtcsm_score_kernel).  *processed as above.
static int launch_score_point(dliom_ctx* ctx, const dliom_cloud& cloud, const GridView& g, const Candidates& c,
                              const DeviceCandidates& d, int r_first, int r_last, unsigned long long* d_sums,
                              int64_t* processed) {
  const int R = static_cast<int>(c.w.num_rotations), T = static_cast<int>(c.w.num_translations);
  const int n = static_cast<int>(cloud.n);
  const int Rs = r_last - r_first;  // rotations of this shard
  int ppt = n >= 32 * 1024 ? 8 : (n >= 8 * 1024 ? 4 : (n >= 2048 ? 2 : 1));
  while (ppt > 1 && (cloud.n_padded % (static_cast<int64_t>(kBlock) * ppt)) != 0) ppt >>= 1;
  const int point_tiles = (n + kBlock * ppt - 1) / (kBlock * ppt);
  int rot_tiles = std::max(1, std::min(Rs, (kScoreTargetBlocks + point_tiles - 1) / point_tiles));
  const int rots_per_block = (Rs + rot_tiles - 1) / rot_tiles;
  rot_tiles = (Rs + rots_per_block - 1) / rots_per_block;
  const size_t lds = static_cast<size_t>(T) * sizeof(unsigned);
  if (lds > 150 * 1024) return DLIOM_ERR_INVALID_ARGUMENT;  // (2L+1)^3 translations must fit LDS
  // bits = 8 (2^33 leaf-table entries): the 64-bit-index kernel is built for 1 and 4 points per lane, on the rotation
  // tiles sized above
  const bool wide = g.log2_leaves > 10;
  const int lane_pts = wide ? (ppt >= 4 ? 4 : 1) : ppt;
  const int tile = kBlock * lane_pts;
  const int tiles = (n + tile - 1) / tile;
  *processed = static_cast<int64_t>(tiles) * tile;
  auto kernel = &rtcsm_score_kernel<1>;
  if (wide) kernel = lane_pts == 4 ? &rtcsm_score_kernel<4, true> : &rtcsm_score_kernel<1, true>;
  else if (lane_pts == 8) kernel = &rtcsm_score_kernel<8>;
  else if (lane_pts == 4) kernel = &rtcsm_score_kernel<4>;
  else if (lane_pts == 2) kernel = &rtcsm_score_kernel<2>;
  const int span = ctx->begin_span(DLIOM_KERNEL_RTCSM_SCORE);
  hipLaunchKernelGGL(kernel, dim3(tiles, rot_tiles), dim3(kBlock), lds, ctx->stream, g, cloud.d_xs, cloud.d_ys, cloud.d_zs,
                     d.rot, R, r_first, r_last, d.trans, T, rots_per_block, d_sums);
  ctx->end_span(span);
  return DLIOM_OK;
}

// Chooses the score kernel (mapping) and launches it; *pad_processed = padding points visited (each adds 1 to every
// sum).  Records the choice in ctx->last_score_mapping / last_box_refusal / last_score_used_box.
static int run_score_volume(dliom_ctx* ctx, const dliom_cloud& cloud, const dliom_grid* grid,
                            const Candidates& c, int r_first, int r_last, DeviceCandidates* d,
                            unsigned long long** d_sums, int64_t* pad_processed, const FillJob* also_fill = nullptr) {
  // candidate tables, the zeroed score volume (and the caller's fill): pending jobs that the first kernel of the chain
  // carries (the box kernel's pre-pass) or one launch of their own (prep_flush) -- not a packet each
  PrepArgs prep;
  prep.n = 0;
  DLIOM_TRY(upload_candidates(ctx, c, d, &prep));
  DLIOM_PREP_LAP(1);
  const int64_t C = c.w.num_candidates;
  DLIOM_TRY(ctx->sums.reserve(static_cast<size_t>(C) * 8));
  *d_sums = ctx->sums.as<unsigned long long>();
  {
    FillJob fills[2] = {{*d_sums, static_cast<size_t>(C) * 8, 0u}, {nullptr, 0, 0u}};
    int nf = 1;
    if (also_fill != nullptr) fills[nf++] = *also_fill;
    for (int k = 0; k < nf; ++k)
      if (!prep_add(&prep, fills[k].p, nullptr, fills[k].bytes, fills[k].value)) DLIOM_TRY(fill_multi(ctx, &fills[k], 1));
  }
  const int T = static_cast<int>(c.w.num_translations);
  const int n = static_cast<int>(cloud.n);
  // 3: LDS-box kernel over the dense mirror (score_box.h; default when the search suits it),
  // 2: rotation per lane over the dense mirror, 1: rotation per lane over the leaf table,
  // 0: point per lane over the leaf table
  int mapping = ctx->tuning[DLIOM_TUNE_SCORE_KERNEL];
  ctx->last_box_refusal = mapping == 3 ? DLIOM_BOX_RAN : DLIOM_BOX_NOT_REQUESTED;
  if (ctx->force_dense_score && mapping > 2) {
    mapping = 2;
    ctx->last_box_refusal = DLIOM_BOX_REFUSED_FLAGGED;  // the box kernel flagged an inconsistency: this is the rerun
  }
  ctx->last_score_used_box = false;
  if (mapping >= 2) {
    // the mirror is a cache of the grid's contents: building it does not change the grid.  Grids beyond bits = 4 get a
    // WINDOW around this match's initial pose that holds every cell the search can read: a rotated point lies within
    // max ||p|| of the candidate's translation, and that within (L + 1) res sqrt(3) of the initial one
    const float res = grid->resolution;
    const int centre[3] = {static_cast<int>(std::lround(c.init.t.x / res)), static_cast<int>(std::lround(c.init.t.y / res)),
                           static_cast<int>(std::lround(c.init.t.z / res))};
    const double reach_cells = static_cast<double>(cloud.max_norm) / res + (c.w.linear_window_size + 1) * 1.7321 + 4.0;
    const int radius = reach_cells < 1.0e6 ? static_cast<int>(std::ceil(reach_cells)) : (1 << 20);
    if (const_cast<dliom_grid*>(grid)->ensure_dense_for(centre, radius) != DLIOM_OK) {
      if (mapping == 3) ctx->last_box_refusal = DLIOM_BOX_REFUSED_NO_MIRROR;
      mapping = 1;  // too large: leaf path
    }
  }
  // a windowed mirror has its own offset per axis: only the box kernel reads it, everything else takes the leaf table
  const bool windowed = grid->dense_windowed;
  if (windowed && mapping == 2) mapping = 1;
  const GridView g = grid->view();
  DLIOM_TRY(ensure_morton(ctx, &cloud));
  DLIOM_PREP_LAP(2);
  if (g.log2_leaves > 10 && mapping >= 1) {  // bits = 8: only the point-per-lane kernel has 64-bit table indices
    if (mapping == 3) ctx->last_box_refusal = DLIOM_BOX_REFUSED_NO_MIRROR;
    mapping = 0;
  }
  if (mapping == 3) {
    const double pairs = static_cast<double>(C) * static_cast<double>(n);
    int s3 = DLIOM_ERR_CAPACITY;
    ctx->last_box_refusal = DLIOM_BOX_REFUSED_SMALL;  // unless the launch below is reached
    if (T >= 8 && pairs >= std::ldexp(1.0, 24)) {  // small searches: launch-bound anyway
      ctx->last_box_refusal = DLIOM_BOX_RAN;
#ifdef DLIOM_EXPERIMENTS
      constexpr size_t kBoxErrorBytes = 256 + 4096 * 32;  // + per-workgroup time stamps (Params::debug & 256)
#else
      constexpr size_t kBoxErrorBytes = 256;
#endif
      DLIOM_TRY(ctx->box_error.reserve(kBoxErrorBytes));
      if (!ctx->box_error_zeroed) {
        DLIOM_HIP_TRY(hipMemsetAsync(ctx->box_error.p, 0, kBoxErrorBytes, ctx->stream));
        ctx->box_error_zeroed = true;
      }
      s3 = launch_score_box(ctx, cloud, g, c, *d, r_first, r_last, *d_sums, ctx->box_error.as<unsigned>(), &prep);
    }
    if (s3 == DLIOM_OK) {
      *pad_processed = 0;
      ctx->last_score_used_box = true;
      ctx->last_score_mapping = 3;
      return DLIOM_OK;
    }
    if (s3 != DLIOM_ERR_CAPACITY) return s3;
    mapping = windowed ? 1 : 2;
  }
  DLIOM_TRY(prep_flush(ctx, &prep));  // the kernels below read the device copies
  ctx->last_score_mapping = mapping;
  int64_t processed = 0;
  if (mapping == 2)
    DLIOM_TRY(launch_score_dense(ctx, cloud, g, c, *d, r_first, r_last, *d_sums, &processed));
  else if (mapping == 1)
    DLIOM_TRY(launch_score_rot(ctx, cloud, g, c, *d, r_first, r_last, *d_sums, &processed));
  else
    DLIOM_TRY(launch_score_point(ctx, cloud, g, c, *d, r_first, r_last, *d_sums, &processed));
  DLIOM_HIP_TRY(hipGetLastError());
  *pad_processed = processed - n;
  return DLIOM_OK;
}

// The affine fit of ValueToProbability (probability_values.h) that the bounds use: |LUT[v] - (a v + b)| <= delta.
struct LutModel {
  double a, b, delta;
};
static const LutModel& lut_model() {
  static const LutModel m = [] {
    LutModel r;
    r.a = static_cast<double>(kValueToProbabilityScale);
    r.b = static_cast<double>(kValueToProbabilityOffset);
    double d = std::fabs(static_cast<double>(kUnknownProbability) - (r.a * 1.0 + r.b));  // value 0 counted as 1
    for (int v = 1; v < 32768; ++v) {
      const float f = v * kValueToProbabilityScale + kValueToProbabilityOffset;
      d = std::max(d, std::fabs(static_cast<double>(f) - (r.a * v + r.b)));
    }
    r.delta = d * 1.0000001 + 1e-12;
    return r;
  }();
  return m;
}

// The LDS-box kernel checks its own fast index against the reference's arithmetic wherever the two could differ; an
// exact cell more than one cell away from the fast one contradicts the error budget of score_box.h ("cannot
// happen").  If it ever does, the kernel sets box_error[0] (sticky, dliom_rtcsm3d_box_error) and box_error[1]: the
// sums are then not trusted and the match is redone with the dense kernel, which has no fast path.
// A test walks this path in a build with -DDLIOM_TEST_HOOKS (libdliom_hooks.so), where knob 2 of dliom_ctx_set_tuning sets the
// word from the host; the library that ships has no such switch.
// `err1` is the word as read back; clears it on the device.
static int box_overflowed(dliom_ctx* ctx, unsigned err1, bool* overflow) {
  *overflow = err1 != 0u;
  if (*overflow)
    DLIOM_HIP_TRY(hipMemsetAsync(static_cast<char*>(ctx->box_error.p) + 4, 0, 4, ctx->stream));
  return DLIOM_OK;
}

// Phase 1: score volume + score bounds for the rotations [shard * R / num_shards, ...).
// local_best_lo_bits (optional) receives this shard's best lower bound (float bits) -- the
// quantity that is max-all-reduced when the window is sharded across GPUs.
static int match_begin(dliom_ctx* ctx, const dliom_rtcsm_options* o, const double init7[7],
                       const dliom_cloud& cloud, const dliom_grid* grid, int shard, int num_shards,
                       unsigned* local_best_lo_bits) {
#ifdef DLIOM_EXPERIMENTS
  g_host_prep.start();
#endif
  if (cloud.n <= 0) return DLIOM_ERR_EMPTY_CLOUD;
  if (cloud.n > (1 << 27) || num_shards < 1 || shard < 0 || shard >= num_shards)
    return DLIOM_ERR_INVALID_ARGUMENT;
  RtcsmState* st = state_of(ctx);
  st->active = false;
  st->o = *o;
  st->cloud = cloud;
  st->grid = grid;
  std::memcpy(st->init7, init7, sizeof st->init7);
  st->shard = shard;
  st->num_shards = num_shards;
  st->used_box = false;
  Candidates& c = st->c;
  generate_candidates(*o, grid->resolution, cloud.max_norm, init7, &c);
  DLIOM_PREP_LAP(0);
  const int64_t C = c.w.num_candidates;
  const int R = static_cast<int>(c.w.num_rotations), T = static_cast<int>(c.w.num_translations);
  if (C <= 0 || C > (int64_t{1} << 31)) return DLIOM_ERR_INVALID_ARGUMENT;
  st->r_first = static_cast<int>(static_cast<int64_t>(R) * shard / num_shards);
  st->r_last = static_cast<int>(static_cast<int64_t>(R) * (shard + 1) / num_shards);

  const size_t bytes_f = align256(static_cast<size_t>(C) * 4);
  DLIOM_TRY(ctx->bounds.reserve(3 * bytes_f + 256));
  char* bb = static_cast<char*>(ctx->bounds.p);
  float* d_lo = reinterpret_cast<float*>(bb);
  st->d_hi = reinterpret_cast<float*>(bb + bytes_f);
  st->d_list = reinterpret_cast<unsigned*>(bb + 2 * bytes_f);
  st->d_ctrs = reinterpret_cast<unsigned*>(bb + 3 * bytes_f);  // [0] best_lo bits, [1] count, [2] arrivals of the read-back
  const FillJob zero_ctrs{st->d_ctrs, 12, 0u};
  if (st->r_last <= st->r_first) DLIOM_TRY(fill_multi(ctx, &zero_ctrs, 1));
  if (st->r_last > st->r_first) {
    int64_t pad_processed = 0;
    DLIOM_TRY(run_score_volume(ctx, cloud, grid, c, st->r_first, st->r_last, &st->d, &st->d_sums,
                               &pad_processed, &zero_ctrs));
    st->used_box = ctx->last_score_used_box;
    const LutModel& lm = lut_model();
    BoundParams bp;
    bp.a = lm.a;
    bp.b = lm.b;
    bp.delta = lm.delta;
    bp.wt = o->translation_delta_cost_weight;
    bp.wr = o->rotation_delta_cost_weight;
    bp.n = static_cast<int>(cloud.n);
    bp.n_pad = static_cast<int>(pad_processed);
    bp.R = R;
    bp.T = T;
    bp.r_first = st->r_first;
    bp.r_last = st->r_last;
    fill_seq_sum_bound_table(bp.n, &bp.err);
    const unsigned cblocks = static_cast<unsigned>((C + 255) / 256);
    const int span = ctx->begin_span(DLIOM_KERNEL_RTCSM_SELECT);
    hipLaunchKernelGGL(rtcsm_bounds_kernel, dim3(cblocks), dim3(256), 0, ctx->stream, st->d_sums,
                       static_cast<long long>(C), st->d.t_norm, st->d.r_angle, bp, d_lo, st->d_hi,
                       st->d_ctrs);
    ctx->end_span(span);
    DLIOM_HIP_TRY(hipGetLastError());
  }
  if (local_best_lo_bits != nullptr) {
    unsigned* h_err = pinned_at<unsigned>(ctx, kPinBoxErrorWord);
    *h_err = 0u;
    DLIOM_HIP_TRY(hipMemcpyAsync(local_best_lo_bits, st->d_ctrs, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (st->used_box)
      DLIOM_HIP_TRY(hipMemcpyAsync(h_err, static_cast<char*>(ctx->box_error.p) + 4, 4, hipMemcpyDeviceToHost, ctx->stream));
    DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    bool overflow = false;
    DLIOM_TRY(box_overflowed(ctx, *h_err, &overflow));
    if (overflow && !ctx->force_dense_score) {
      ctx->force_dense_score = true;
      const dliom_rtcsm_options o_copy = st->o;
      const int s = match_begin(ctx, &o_copy, init7, cloud, grid, shard, num_shards, local_best_lo_bits);
      ctx->force_dense_score = false;
      return s;
    }
  }
  st->active = true;
  return DLIOM_OK;
}

// Phase 2: survivors against the (global) best lower bound, exact sequential rescoring, and this
// shard's winner packed as (score_bits << 32) | (0xFFFFFFFF - index): the max over shards of that
// word is the reference's first-maximum-in-generation-order winner.
static int match_finish(dliom_ctx* ctx, const unsigned* global_best_lo_bits, uint64_t* local_best_packed) {
  RtcsmState* st = state_of(ctx);
  if (!st->active) return DLIOM_ERR_INVALID_ARGUMENT;
  const dliom_rtcsm_options* o = &st->o;
  const Candidates& c = st->c;
  const int64_t C = c.w.num_candidates;
  const int R = static_cast<int>(c.w.num_rotations);
  const dliom_cloud& cloud = st->cloud;
  st->best_score = -1.f;
  st->best_c = -1;
  unsigned K = 0;
  if (st->r_last > st->r_first) {
    if (global_best_lo_bits != nullptr) {
      DLIOM_HIP_TRY(hipMemcpyAsync(st->d_ctrs, global_best_lo_bits, 4, hipMemcpyHostToDevice, ctx->stream));
    }
    const unsigned cblocks = static_cast<unsigned>((C + 255) / 256);
    int span = ctx->begin_span(DLIOM_KERNEL_RTCSM_SELECT);
    hipLaunchKernelGGL(rtcsm_select_kernel, dim3(cblocks), dim3(256), 0, ctx->stream, st->d_hi,
                       static_cast<long long>(C), st->d_ctrs, st->d_ctrs + 1, st->d_list);
    ctx->end_span(span);
    DLIOM_HIP_TRY(hipGetLastError());
  }
  // Exact sequential rescoring of the survivors, one workgroup each.  Usually a handful survive, so
  // the first kSpecK are rescored SPECULATIVELY in the same stream segment (the kernels read the
  // count on the device and idle blocks exit): one synchronisation for the whole match.  Only if
  // more survived does a second, exactly sized round run.
  constexpr unsigned kSpecK = 8;
  std::vector<unsigned> list;
  std::vector<float> ksums;
  if (st->r_last > st->r_first) {
    // readback block: [count pair | list | sums | box overflow word]
    static_assert((2 + 2 * kSpecK + 1) * 4 <= kPinMatchReadback.bytes, "the read-back fits its region");
    unsigned* h_ctrs = pinned_at<unsigned>(ctx, kPinMatchReadback);
    unsigned* h_list = h_ctrs + 2;
    float* h_sums = reinterpret_cast<float*>(h_ctrs + 2 + kSpecK);
    auto rescore = [&](unsigned count, const unsigned* d_count, size_t list_offset, const SumReadback* readback) -> int {
      DLIOM_TRY(ctx->rescore.reserve(align256(static_cast<size_t>(count) * 4)));
      const int span = ctx->begin_span(DLIOM_KERNEL_RTCSM_RESCORE);
      const int s = launch_sequential_sums(ctx, sequential_sum_method(cloud.n), st->grid->view(), cloud, st->d.rot, R, st->d.trans,
                                           st->d_list + list_offset, d_count, count, &ctx->misc, ctx->rescore.as<float>(), readback);
      ctx->end_span(span);
      return s;
    };
    // the read-back [count pair | list | sums | box overflow word] is written by the last rescoring kernel itself
    // (SumReadback, sequential_sums.hip): no gather launch behind it.  The chain in front of the completion word is the
    // whole match, so the word is polled for twice as long as the previous match's wait took (150 us .. 4 ms).
    unsigned* h_err = h_ctrs + 2 + 2 * kSpecK;
    *h_err = 0u;
    const bool want_err = st->used_box && global_best_lo_bits == nullptr;
    if (ctx->done_word != nullptr) {
      SumReadback rb;
      rb.dst = h_ctrs;
      rb.ctrs = st->d_ctrs;
      rb.err_word = want_err ? reinterpret_cast<const unsigned*>(static_cast<char*>(ctx->box_error.p) + 4) : nullptr;
      rb.arrivals = st->d_ctrs + 2;
      rb.done_word = ctx->done_word;
      rb.done_seq = next_done_seq(ctx);
      rb.slots = kSpecK;
      DLIOM_TRY(rescore(kSpecK, st->d_ctrs + 1, 0, &rb));
      const auto t0 = std::chrono::steady_clock::now();
      const int s = wait_done(ctx, ctx->stream, ctx->done_word, rb.done_seq, ctx->match_poll_us);
      const double took_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      ctx->match_poll_us = static_cast<int>(std::min(4000.0, std::max(150.0, 2.0 * took_us)));
      DLIOM_TRY(s);
    } else {  // no completion word (allocation failed at creation): a gather and a synchronise
      DLIOM_TRY(rescore(kSpecK, st->d_ctrs + 1, 0, nullptr));
      const GatherJob back[4] = {{st->d_ctrs, 2}, {st->d_list, kSpecK}, {ctx->rescore.p, kSpecK},
                                 {static_cast<char*>(ctx->box_error.p) + 4, 1}};
      DLIOM_TRY(gather_and_wait(ctx, back, want_err ? 4 : 3, h_ctrs));
    }
    {
      bool overflow = false;
      DLIOM_TRY(box_overflowed(ctx, *h_err, &overflow));
      if (overflow && !ctx->force_dense_score) {  // redo the whole match on the dense kernel
        ctx->force_dense_score = true;
        const dliom_rtcsm_options o_copy = st->o;
        const dliom_cloud cloud_copy = st->cloud;
        double init_copy[7];
        std::memcpy(init_copy, st->init7, sizeof init_copy);
        int s = match_begin(ctx, &o_copy, init_copy, cloud_copy, st->grid, st->shard, st->num_shards, nullptr);
        if (s == DLIOM_OK) s = match_finish(ctx, nullptr, local_best_packed);
        ctx->force_dense_score = false;
        return s;
      }
    }
    K = h_ctrs[1];
    const unsigned first = std::min(K, kSpecK);
    list.assign(h_list, h_list + first);
    ksums.assign(h_sums, h_sums + first);
    if (K > kSpecK) {  // the rest, exactly sized
      const unsigned rest = K - kSpecK;
      DLIOM_TRY(rescore(rest, nullptr, kSpecK, nullptr));
      list.resize(K);
      ksums.resize(K);
      DLIOM_HIP_TRY(hipMemcpyAsync(list.data() + kSpecK, st->d_list + kSpecK, static_cast<size_t>(rest) * 4,
                                   hipMemcpyDeviceToHost, ctx->stream));
      DLIOM_HIP_TRY(hipMemcpyAsync(ksums.data() + kSpecK, ctx->rescore.p, static_cast<size_t>(rest) * 4,
                                   hipMemcpyDeviceToHost, ctx->stream));
      DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
  }
  if (K > 0) {
    const int n = static_cast<int>(cloud.n);
    // final scoring exactly as rtcsm_3d.cc:105-112, first maximum in generation order
    for (unsigned k = 0; k < K; ++k) {
      const int64_t cc = list[k];
      const int j = static_cast<int>(cc / R), r = static_cast<int>(cc % R);
      float score = ksums[k];
      score /= static_cast<float>(n);
      const double arg = c.t_norm[j] * o->translation_delta_cost_weight +
                         c.r_angle[r] * o->rotation_delta_cost_weight;
      score *= std::exp(-(arg * (arg * 1.0)));
      if (score > st->best_score || (score == st->best_score && cc < st->best_c)) {
        st->best_score = score;
        st->best_c = cc;
      }
    }
  }
  ctx->last_rtcsm.window = c.w;
  ctx->last_rtcsm.num_points = cloud.n;
  ctx->last_rtcsm.num_rescored = K;
  ctx->last_rtcsm.score_kernel = ctx->last_score_mapping;
  ctx->last_rtcsm.box_kernel_status = ctx->last_box_refusal;
  ctx->last_rtcsm.box_kernel_variant = ctx->last_box_refusal == DLIOM_BOX_RAN ? ctx->last_box_variant : -1;
  ctx->last_rtcsm.best_index = st->best_c;
  if (local_best_packed != nullptr) {
    uint64_t packed = 0;  // a shard without a positive-score survivor contributes nothing
    if (st->best_c >= 0 && st->best_score > 0.f) {
      uint32_t bits;
      std::memcpy(&bits, &st->best_score, 4);
      packed = (static_cast<uint64_t>(bits) << 32) | (0xFFFFFFFFull - static_cast<uint64_t>(st->best_c));
    }
    *local_best_packed = packed;
  }
  return DLIOM_OK;
}

// Phase 3: pose of the winning candidate (every shard can decode it: candidates are replicated).
static int match_decode(dliom_ctx* ctx, uint64_t best_packed, double out7[7], float* out_score) {
  RtcsmState* st = state_of(ctx);
  if (!st->active) return DLIOM_ERR_INVALID_ARGUMENT;
  if (best_packed == 0) return DLIOM_ERR_SCORE_NOT_POSITIVE;  // CHECK_GT(score, 0.f)
  const Candidates& c = st->c;
  const int R = static_cast<int>(c.w.num_rotations);
  const uint32_t bits = static_cast<uint32_t>(best_packed >> 32);
  const int64_t best_c = static_cast<int64_t>(0xFFFFFFFFull - (best_packed & 0xFFFFFFFFull));
  if (best_c < 0 || best_c >= c.w.num_candidates) return DLIOM_ERR_INVALID_ARGUMENT;
  float score;
  std::memcpy(&score, &bits, 4);
  const int j = static_cast<int>(best_c / R), r = static_cast<int>(best_c % R);
  out7[0] = c.trans[j].x;
  out7[1] = c.trans[j].y;
  out7[2] = c.trans[j].z;
  const QF q = c.rot(static_cast<size_t>(r));  // the table's entry, bit for bit (rtcsm_candidates.h)
  out7[3] = q.w;
  out7[4] = q.x;
  out7[5] = q.y;
  out7[6] = q.z;
  *out_score = score;
  ctx->last_rtcsm.best_index = best_c;
  return DLIOM_OK;
}

static int match_impl(dliom_ctx* ctx, const dliom_rtcsm_options* o, const double init7[7],
                      const dliom_cloud& cloud, const dliom_grid* grid, double out7[7],
                      float* out_score) {
  DLIOM_TRY(match_begin(ctx, o, init7, cloud, grid, 0, 1, nullptr));
  uint64_t packed = 0;
  DLIOM_TRY(match_finish(ctx, nullptr, &packed));
  return match_decode(ctx, packed, out7, out_score);
}

}  // namespace dliom

using namespace dliom;

extern "C" {

int dliom_rtcsm3d_window(const dliom_rtcsm_options* o, float resolution, const float* points_xyz,
                         int64_t n, dliom_rtcsm_window* w) {
  if (o == nullptr || w == nullptr || n < 0 || (n > 0 && points_xyz == nullptr))
    return DLIOM_ERR_INVALID_ARGUMENT;
  compute_window(*o, resolution, cloud_max_norm(points_xyz, n), w);
  return DLIOM_OK;
}

int dliom_rtcsm3d_match_cloud(dliom_ctx* ctx, const dliom_rtcsm_options* o, const double init7[7],
                              const dliom_cloud* cloud, const dliom_grid* grid, double out7[7],
                              float* score) {
  if (ctx == nullptr || o == nullptr || init7 == nullptr || cloud == nullptr || grid == nullptr ||
      out7 == nullptr || score == nullptr)
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  return match_impl(ctx, o, init7, *cloud, grid, out7, score);
}

int dliom_rtcsm3d_match(dliom_ctx* ctx, const dliom_rtcsm_options* o, const double init7[7],
                        const float* points_xyz, int64_t n, const dliom_grid* grid, double out7[7],
                        float* score) {
  if (ctx == nullptr || o == nullptr || init7 == nullptr || grid == nullptr || out7 == nullptr ||
      score == nullptr || n < 0 || (n > 0 && points_xyz == nullptr))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (n == 0) return DLIOM_ERR_EMPTY_CLOUD;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(ctx->points.reserve(staged_cloud_bytes(n)));
  dliom_cloud cloud;
  DLIOM_TRY(stage_cloud(ctx, points_xyz, n, &cloud));
  return match_impl(ctx, o, init7, cloud, grid, out7, score);
}

int dliom_rtcsm3d_shard_begin(dliom_ctx* ctx, const dliom_rtcsm_options* o, const double init7[7],
                              const dliom_cloud* cloud, const dliom_grid* grid, int shard, int num_shards,
                              uint32_t* local_best_lower_bound_bits) {
  if (ctx == nullptr || o == nullptr || init7 == nullptr || cloud == nullptr || grid == nullptr ||
      local_best_lower_bound_bits == nullptr)
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  return match_begin(ctx, o, init7, *cloud, grid, shard, num_shards, local_best_lower_bound_bits);
}

int dliom_rtcsm3d_shard_finish(dliom_ctx* ctx, uint32_t global_best_lower_bound_bits,
                               uint64_t* local_best_packed) {
  if (ctx == nullptr || local_best_packed == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  return match_finish(ctx, &global_best_lower_bound_bits, local_best_packed);
}

int dliom_rtcsm3d_shard_decode(dliom_ctx* ctx, uint64_t global_best_packed, double pose_estimate[7],
                               float* score) {
  if (ctx == nullptr || pose_estimate == nullptr || score == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  return match_decode(ctx, global_best_packed, pose_estimate, score);
}

// ---- config 4: the search window sharded over the ranks of a node, ONE 8-byte collective per match --------------
// Every rank scores its own contiguous range of candidate rotations and finds ITS winner exactly (own bounds, own
// exact rescoring).  The global winner -- the reference's first strictly greater score in generation order
// (rtcsm_3d.cc:46-51) -- is the maximum of the ranks' packed words (score_bits << 32 | ~index): positive floats order
// like their bit patterns and the complemented index lets the lower index win ties.  One MAX all-reduce of one
// uint64; its 8 bytes are latency, not bandwidth.  The three-phase calls above stay for callers that
// want the global lower bound exchanged first (less rescoring per rank, two collectives).
// reserved word of a rank that failed: above every real packed word (score bits of a finite positive float are at most
// 0x7F7FFFFF) under unsigned AND signed 64-bit MAX -- torch.distributed has no uint64, callers reduce int64
static constexpr uint64_t kShardFailed = 0x7FFFFFFFFFFFFFFFull;
int dliom_rtcsm3d_match_sharded(dliom_ctx* ctx, const dliom_rtcsm_options* o, const double init7[7], const dliom_cloud* cloud,
                                const dliom_grid* grid, int shard, int num_shards, dliom_allreduce_max_u64 exchange,
                                void* user, double out7[7], float* score) {
  if (num_shards > 1 && exchange == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  // Every rank ALWAYS takes part in the exchange: a rank that failed locally (bad arguments, a HIP error, an
  // allocation, a refusal, an empty cloud) contributes the reserved word kShardFailed -- the maximum, so every rank
  // sees it -- and returns its own status afterwards; the others return DLIOM_ERR_PEER_FAILED.  Returning before the
  // collective would leave the peers blocked in it (on RCCL: a device-side hang without an error).
  int local = ctx == nullptr || o == nullptr || init7 == nullptr || cloud == nullptr || grid == nullptr || out7 == nullptr ||
                      score == nullptr
                  ? DLIOM_ERR_INVALID_ARGUMENT
                  : DLIOM_OK;
  if (local == DLIOM_OK && hipSetDevice(ctx->device) != hipSuccess) local = DLIOM_ERR_HIP;
  uint64_t packed = 0;
  if (local == DLIOM_OK) local = match_begin(ctx, o, init7, *cloud, grid, shard, num_shards, nullptr);
  if (local == DLIOM_OK) local = match_finish(ctx, nullptr, &packed);
  if (local != DLIOM_OK) packed = kShardFailed;
  if (num_shards > 1 && exchange(&packed, user) != 0) return local != DLIOM_OK ? local : DLIOM_ERR_HIP;
  if (local != DLIOM_OK) return local;
  if (packed == kShardFailed) return DLIOM_ERR_PEER_FAILED;
  return match_decode(ctx, packed, out7, score);
}

}  // extern "C"

namespace {
struct RcclApi {
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  bool ok = false;
};
// librccl is looked up when the first sharded match runs: libdliom.so itself loads (and every other entry point
// works) on machines without RCCL.
const RcclApi& rccl_api() {
  static const RcclApi api = [] {
    RcclApi a;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (h == nullptr) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (h == nullptr) return a;
    a.CommCount = reinterpret_cast<decltype(a.CommCount)>(dlsym(h, "ncclCommCount"));
    a.CommUserRank = reinterpret_cast<decltype(a.CommUserRank)>(dlsym(h, "ncclCommUserRank"));
    a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(h, "ncclAllReduce"));
    a.ok = a.CommCount != nullptr && a.CommUserRank != nullptr && a.AllReduce != nullptr;
    return a;
  }();
  return api;
}
struct RcclExchange {
  dliom_ctx* ctx;
  ncclComm_t comm;
};
int rccl_exchange(uint64_t* value, void* user) {
  RcclExchange* x = static_cast<RcclExchange*>(user);
  dliom_ctx* ctx = x->ctx;
  if (ctx->misc.reserve(256) != DLIOM_OK) return 1;
  uint64_t* d = ctx->misc.as<uint64_t>();
  uint64_t* h = pinned_at<uint64_t>(ctx, kPinRcclWord);
  *h = *value;
  const int span = ctx->begin_span(DLIOM_KERNEL_ALLREDUCE);  // (profiling on: HIP events around the collective)
  bool ok = hipMemcpyAsync(d, h, 8, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
            rccl_api().AllReduce(d, d, 1, ncclUint64, ncclMax, x->comm, ctx->stream) == ncclSuccess &&
            hipMemcpyAsync(h, d, 8, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
  ctx->end_span(span);
  if (!ok) return 1;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return 1;
  *value = *h;
  return 0;
}
}  // namespace

extern "C" {

int dliom_rtcsm3d_match_sharded_rccl(dliom_ctx* ctx, const dliom_rtcsm_options* o, const double init7[7],
                                     const dliom_cloud* cloud, const dliom_grid* grid, void* nccl_comm, double out7[7],
                                     float* score) {
  if (ctx == nullptr || nccl_comm == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  const RcclApi& api = rccl_api();
  if (!api.ok) {
    set_last_error("dlopen(librccl.so.1): RCCL not available", hipErrorSharedObjectInitFailed, __FILE__, __LINE__);
    return DLIOM_ERR_HIP;
  }
  int rank = 0, size = 1;
  ncclComm_t comm = static_cast<ncclComm_t>(nccl_comm);
  if (api.CommCount(comm, &size) != ncclSuccess || api.CommUserRank(comm, &rank) != ncclSuccess) return DLIOM_ERR_INVALID_ARGUMENT;
  RcclExchange x{ctx, comm};
  // a communicator of one rank still goes through ncclAllReduce (size 1 is a copy): same code path as on 8 GPUs
  if (size == 1) {
    if (ctx == nullptr || o == nullptr || init7 == nullptr || cloud == nullptr || grid == nullptr || out7 == nullptr ||
        score == nullptr)
      return DLIOM_ERR_INVALID_ARGUMENT;
    int local = hipSetDevice(ctx->device) == hipSuccess ? DLIOM_OK : DLIOM_ERR_HIP;
    uint64_t packed = 0;
    if (local == DLIOM_OK) local = match_begin(ctx, o, init7, *cloud, grid, 0, 1, nullptr);
    if (local == DLIOM_OK) local = match_finish(ctx, nullptr, &packed);
    if (local != DLIOM_OK) packed = kShardFailed;
    if (rccl_exchange(&packed, &x) != 0) return local != DLIOM_OK ? local : DLIOM_ERR_HIP;
    if (local != DLIOM_OK) return local;
    return match_decode(ctx, packed, out7, score);
  }
  return dliom_rtcsm3d_match_sharded(ctx, o, init7, cloud, grid, rank, size, rccl_exchange, &x, out7, score);
}

int dliom_rtcsm3d_box_error(dliom_ctx* ctx, uint32_t* flags) {
  if (ctx == nullptr || flags == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *flags = 0;
  if (ctx->box_error.p == nullptr) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_HIP_TRY(hipMemcpyAsync(flags, ctx->box_error.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DLIOM_OK;
}

#ifdef DLIOM_EXPERIMENTS
// experiments builds only (not in dliom.h): the box kernel's work counters (Params::debug & 128), read and cleared
extern "C" int dliom_exp_box_stats(dliom_ctx* ctx, uint32_t out[8]) {
  if (ctx == nullptr || out == nullptr || ctx->box_error.p == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipMemcpyAsync(out, static_cast<char*>(ctx->box_error.p) + 32, 32, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipMemsetAsync(static_cast<char*>(ctx->box_error.p) + 32, 0, 32, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DLIOM_OK;
}
#endif

#ifdef DLIOM_EXPERIMENTS
// per-workgroup stamps of the last box-kernel launch: (start, end) in 10 ns ticks, tickets processed, XCC id
extern "C" int dliom_exp_box_stamps(dliom_ctx* ctx, uint64_t* out, int workgroups) {
  if (ctx == nullptr || out == nullptr || ctx->box_error.p == nullptr || workgroups > 4096) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipMemcpyAsync(out, static_cast<char*>(ctx->box_error.p) + 256, static_cast<size_t>(workgroups) * 32,
                               hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DLIOM_OK;
}
#endif

int dliom_rtcsm3d_last_stats(const dliom_ctx* ctx, dliom_rtcsm_stats* stats) {
  if (ctx == nullptr || stats == nullptr) return DLIOM_ERR_INVALID_ARGUMENT;
  *stats = ctx->last_rtcsm;
  return DLIOM_OK;
}

int dliom_rtcsm3d_score_volume(dliom_ctx* ctx, const dliom_rtcsm_options* o, const double init7[7],
                               const float* points_xyz, int64_t n, const dliom_grid* grid,
                               uint64_t* sums, int64_t capacity, int64_t* num_candidates) {
  if (ctx == nullptr || o == nullptr || init7 == nullptr || grid == nullptr ||
      num_candidates == nullptr || n <= 0 || points_xyz == nullptr)
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(ctx->points.reserve(staged_cloud_bytes(n)));
  dliom_cloud cloud;
  DLIOM_TRY(stage_cloud(ctx, points_xyz, n, &cloud));
  Candidates c;
  generate_candidates(*o, grid->resolution, cloud.max_norm, init7, &c);
  *num_candidates = c.w.num_candidates;
  if (sums == nullptr) return DLIOM_OK;
  if (capacity < c.w.num_candidates) return DLIOM_ERR_CAPACITY;
  DeviceCandidates d;
  unsigned long long* d_sums = nullptr;
  int64_t pad_processed = 0;
  DLIOM_TRY(run_score_volume(ctx, cloud, grid, c, 0, static_cast<int>(c.w.num_rotations), &d, &d_sums,
                             &pad_processed));
  unsigned err1 = 0u;
  if (ctx->last_score_used_box)
    DLIOM_HIP_TRY(hipMemcpyAsync(&err1, static_cast<char*>(ctx->box_error.p) + 4, 4, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipMemcpyAsync(sums, d_sums, static_cast<size_t>(c.w.num_candidates) * 8,
                               hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  {
    bool overflow = false;
    DLIOM_TRY(box_overflowed(ctx, err1, &overflow));
    if (overflow) {
      ctx->force_dense_score = true;
      const int s = run_score_volume(ctx, cloud, grid, c, 0, static_cast<int>(c.w.num_rotations), &d, &d_sums, &pad_processed);
      ctx->force_dense_score = false;
      DLIOM_TRY(s);
      DLIOM_HIP_TRY(hipMemcpyAsync(sums, d_sums, static_cast<size_t>(c.w.num_candidates) * 8, hipMemcpyDeviceToHost, ctx->stream));
      DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
  }
  const uint64_t n_pad = static_cast<uint64_t>(pad_processed);
  for (int64_t i = 0; i < c.w.num_candidates; ++i) sums[i] -= n_pad;
  return DLIOM_OK;
}

int dliom_rtcsm3d_sequential_sums(dliom_ctx* ctx, const dliom_rtcsm_options* o, const double init7[7],
                                  const float* points_xyz, int64_t n, const dliom_grid* grid,
                                  const int64_t* candidate_indices, int64_t k, int method, float* sums) {
  if (ctx == nullptr || o == nullptr || init7 == nullptr || grid == nullptr || candidate_indices == nullptr ||
      sums == nullptr || n <= 0 || points_xyz == nullptr || k <= 0)
    return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(ctx->points.reserve(staged_cloud_bytes(n)));
  dliom_cloud cloud;
  DLIOM_TRY(stage_cloud(ctx, points_xyz, n, &cloud));
  Candidates c;
  generate_candidates(*o, grid->resolution, cloud.max_norm, init7, &c);
  DeviceCandidates d;
  DLIOM_TRY(upload_candidates(ctx, c, &d));
  std::vector<unsigned> list(static_cast<size_t>(k));
  for (int64_t i = 0; i < k; ++i) {
    if (candidate_indices[i] < 0 || candidate_indices[i] >= c.w.num_candidates) return DLIOM_ERR_INVALID_ARGUMENT;
    list[i] = static_cast<unsigned>(candidate_indices[i]);
  }
  const size_t lbytes = align256(static_cast<size_t>(k) * 4);
  DLIOM_TRY(ctx->rescore.reserve(2 * lbytes));
  unsigned* d_list = ctx->rescore.as<unsigned>();
  float* d_ksums = reinterpret_cast<float*>(static_cast<char*>(ctx->rescore.p) + lbytes);
  DLIOM_HIP_TRY(hipMemcpyAsync(d_list, list.data(), static_cast<size_t>(k) * 4, hipMemcpyHostToDevice, ctx->stream));
  const int R = static_cast<int>(c.w.num_rotations);
  if (method < 0 || method > 2 || k > 65535) return DLIOM_ERR_INVALID_ARGUMENT;
  if (method != 0 && ((static_cast<size_t>(n) + 7) & ~static_cast<size_t>(7)) * 2 > 128 * 1024) return DLIOM_ERR_INVALID_ARGUMENT;
  DLIOM_TRY(launch_sequential_sums(ctx, method, grid->view(), cloud, d.rot, R, d.trans, d_list, nullptr,
                                   static_cast<unsigned>(k), &ctx->misc, d_ksums));
  DLIOM_HIP_TRY(hipMemcpyAsync(sums, d_ksums, static_cast<size_t>(k) * 4, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DLIOM_OK;
}

int dliom_probe_transform_cell_indices(dliom_ctx* ctx, const float pose[7], const float* points_xyz,
                                       int64_t n, float resolution, int32_t* cell_xyz) {
  if (ctx == nullptr || pose == nullptr || n < 0 || (n > 0 && (points_xyz == nullptr || cell_xyz == nullptr)))
    return DLIOM_ERR_INVALID_ARGUMENT;
  if (n == 0) return DLIOM_OK;
  DLIOM_HIP_TRY(hipSetDevice(ctx->device));
  DLIOM_TRY(ctx->points.reserve(staged_cloud_bytes(n)));
  dliom_cloud cloud;
  DLIOM_TRY(stage_cloud(ctx, points_xyz, n, &cloud));
  DLIOM_TRY(ctx->misc.reserve(static_cast<size_t>(n) * 12));
  int* d_out = ctx->misc.as<int>();
  const Quat4 q{pose[3], pose[4], pose[5], pose[6]};
  hipLaunchKernelGGL(probe_cells_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0,
                     ctx->stream, q, pose[0], pose[1], pose[2], cloud.d_x, cloud.d_y, cloud.d_z,
                     static_cast<int>(n), resolution, d_out);
  DLIOM_HIP_TRY(hipGetLastError());
  DLIOM_HIP_TRY(hipMemcpyAsync(cell_xyz, d_out, static_cast<size_t>(n) * 12, hipMemcpyDeviceToHost,
                               ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DLIOM_OK;
}

}  // extern "C"
