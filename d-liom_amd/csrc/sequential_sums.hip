// Exact sequential float sums of LUT probabilities on gfx950: the bit-identical replay of the reference's
// `score += probability` loops (real_time_correlative_scan_matcher_3d.cc:101-104, low_resolution_matcher.cc:27-34).
//
// A service with four clients: the survivors of the real-time matcher (rtcsm3d.hip match_finish), the loop-closure
// matcher's low-resolution check and the batched constraint path (fast_csm3d.hip), and the diagnostic ABI call
// dliom_rtcsm3d_sequential_sums.  Three methods that return identical bits (test_sequential_sum_kernels_bit_exact):
//   0  one lane replays the loop (rtcsm_rescore_kernel)
//   1  element scan, binade by binade (rtcsm_rescore_values_kernel + rtcsm_rescore_scan_kernel)
//   2  chunk functions + binade-wise scan (... + rtcsm_rescore_chunk_fns_kernel + rtcsm_rescore_chunk_scan_kernel)
// The kernels keep the rtcsm_rescore_ names they had in rtcsm3d.hip: committed kernel statistics refer to them.
//
// Method 2's scan kernel walks the sum binade by binade on TWO levels, all of it on wave 0 and without a block barrier:
// a chunk is 64 additions with a ParityFn per binade the sum can be in while it crosses the chunk (ChunkFns, at most two),
// a super-chunk is 64 consecutive chunks (4 096 additions) whose ParityFn for a binade is the composition of its chunks'
// functions in chunk order -- defined only where all 64 chunks carry one (at most two binades again; wave w builds
// super-chunk w with one wave scan per binade, behind the kernel's first barrier).  Composition is associative, so a pass
// that skips whole super-chunks (lane <-> super-chunk), opens the one that halts it lane <-> chunk and the crossing chunk
// lane <-> element ends in the same (m, e, i0) as one that composes the chunks one by one.  Whatever the one-wave walk does
// not handle -- a chunk without a function for the binade in front of the crossing, i.e. a violated bound -- is left
// with its exact state to the block's pass (sixteen waves, chunk per thread; sh_force_serial opens such chunks element
// by element), which is also what methods 0 and 1 are compared with.
//
// A client that wants the sums on the host (the real-time matcher) passes a SumReadback: the blocks of the last kernel
// then write their own list word and sum into the page-locked block, and the last block to arrive -- blocks beyond the
// live count arrive too -- adds the count pair, the box overflow word and the completion word.  Nobody waits for anybody.
#include <algorithm>
#include <cstring>
#include <vector>

#include "device_common.h"
#include "probability_values.h"

namespace dliom {

// One thread of every block of a sum's last kernel: its own list word and sum into the read-back block (has_sum: the block
// is below the live count), then the arrival; the last one adds what no block owns and releases the host.  The counter is
// re-armed for the next launch, as csm_final_reduce_kernel does.
__device__ __forceinline__ void publish_sum(const SumReadback& rb, const unsigned* __restrict__ list, bool has_sum, float sum) {
  if (rb.dst == nullptr) return;
  const unsigned k = blockIdx.x;
  if (has_sum && k < rb.slots) {
    rb.dst[2u + k] = list[k];
    rb.dst[2u + rb.slots + k] = __float_as_uint(sum);
  }
  __threadfence_system();
  if (atomicAdd(rb.arrivals, 1u) == gridDim.x - 1u) {
    *rb.arrivals = 0u;
    rb.dst[0] = rb.ctrs[0];
    rb.dst[1] = rb.ctrs[1];
    if (rb.err_word != nullptr) rb.dst[2u + 2u * rb.slots] = *rb.err_word;
    __threadfence_system();
    *reinterpret_cast<volatile unsigned*>(rb.done_word) = rb.done_seq;
  }
}

// ---------------------------------------------------------------------------------- kernel C
// One workgroup per surviving candidate.  Waves 1-3 turn tiles of points (INPUT order) into
// probabilities in LDS -- ValueToProbability(value) as probability_values.cc:27-36 computes it:
// value * kScale + (kMin - kScale), 0 -> kMin -- while lane 0 of wave 0 replays the reference's
// `score += probability` loop (rtcsm_3d.cc:101-104) over the previous tile: strictly sequential
// float additions in point order, so the sum is bit-identical to the reference's.
constexpr int kChainTile = 2048;
__global__ __launch_bounds__(256) void rtcsm_rescore_kernel(
    GridView g, const float* __restrict__ px, const float* __restrict__ py,
    const float* __restrict__ pz, int n, const float4* __restrict__ rot, int R,
    const float* __restrict__ trans, const unsigned* __restrict__ list, const unsigned* __restrict__ count,
    float k_scale, float k_offset, float k_unknown, float* __restrict__ sums, SumReadback rb) {
  __shared__ float4 tile[2][kChainTile / 4];
  if (count != nullptr && blockIdx.x >= *count) {
    if (threadIdx.x == 0) publish_sum(rb, list, false, 0.f);
    return;
  }
  const unsigned c = list[blockIdx.x];
  const int j = static_cast<int>(c / static_cast<unsigned>(R));
  const int r = static_cast<int>(c % static_cast<unsigned>(R));
  const float4 qq = rot[r];
  const Quat4 q{qq.x, qq.y, qq.z, qq.w};
  const float tx = trans[3 * j], ty = trans[3 * j + 1], tz = trans[3 * j + 2];
  const int num_tiles = (n + kChainTile - 1) / kChainTile;
  const int producer = static_cast<int>(threadIdx.x) - 64;  // waves 1..3
  auto produce = [&](int t) {
    if (producer < 0) return;
    float* dst = reinterpret_cast<float*>(tile[t & 1]);
    for (int k = producer; k < kChainTile; k += 192) {
      const int i = t * kChainTile + k;
      float prob = 0.f;  // +0.f padding leaves a float running sum unchanged
      if (i < n) {
        float rx, ry, rz;
        rotate_point(q, px[i], py[i], pz[i], rx, ry, rz);
        const unsigned v = grid_value(g, cell_of(rx + tx, g.resolution), cell_of(ry + ty, g.resolution),
                                      cell_of(rz + tz, g.resolution)) & 0x7FFFu;
        prob = v == 0u ? k_unknown : static_cast<float>(static_cast<int>(v)) * k_scale + k_offset;
      }
      dst[k] = prob;
    }
  };
  float s = 0.f;
  produce(0);
  __syncthreads();
  for (int t = 0; t < num_tiles; ++t) {
    if (t + 1 < num_tiles) produce(t + 1);
    if (threadIdx.x == 0) {
      const float4* src = tile[t & 1];
#pragma unroll 8
      for (int k = 0; k < kChainTile / 4; ++k) {
        const float4 v = src[k];
        s += v.x;
        s += v.y;
        s += v.z;
        s += v.w;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sums[blockIdx.x] = s;
    publish_sum(rb, list, true, s);
  }
}

// Parallel, bit-exact evaluation of the SAME sequential float sum (one workgroup of 1024 threads
// per surviving candidate).  Float addition is not associative, but inside one binade it is
// integer arithmetic: with the running sum s = m * U (U = ulp of the binade, m a 24-bit mantissa)
// and every addend an exact multiple of 2^-27,
//     fl(s + a) = (m + c) * U,   c = floor(a/U) + [frac(a/U) > 1/2]   (+ ties-to-even),
// so a stretch of additions that stays in one binade is an exact integer prefix sum.  Ties
// (frac == 1/2) depend on the parity of m, which a tie itself resets to even; that makes every
// segment of addends a function {parity in} -> {increment, parity out}, and functions compose
// associatively -> a block-wide scan.  The sum is therefore computed binade by binade: each pass
// scans a window that must contain the next binade crossing, finds the first addition whose
// result reaches 2^24 U, rounds that one exact sum to the new ulp 2U, and continues behind it.
// The first 256 additions are simply replayed in float by one lane.
struct ParityFn {
  unsigned s0, s1;  // total increment for parity-in 0 / 1
  unsigned p0, p1;  // parity out
};
__device__ __forceinline__ ParityFn compose(const ParityFn& a, const ParityFn& b) {  // a first, then b
  ParityFn r;
  r.s0 = a.s0 + (a.p0 ? b.s1 : b.s0);
  r.p0 = a.p0 ? b.p1 : b.p0;
  r.s1 = a.s1 + (a.p1 ? b.s1 : b.s0);
  r.p1 = a.p1 ? b.p1 : b.p0;
  return r;
}
__device__ __forceinline__ ParityFn shfl_up_fn(const ParityFn& f, int off) {
  ParityFn r;
  r.s0 = __shfl_up(f.s0, off, 64);
  r.s1 = __shfl_up(f.s1, off, 64);
  r.p0 = __shfl_up(f.p0, off, 64);
  r.p1 = __shfl_up(f.p1, off, 64);
  return r;
}

constexpr int kScanThreads = 1024;
constexpr int kSerialPrefix = 256;

// Per survivor k and point i (input order): the 15-bit grid value, for the scan kernel below.
__global__ void rtcsm_rescore_values_kernel(GridView g, const float* __restrict__ px,
                                            const float* __restrict__ py, const float* __restrict__ pz,
                                            int n, int n_stride, const float4* __restrict__ rot, int R,
                                            const float* __restrict__ trans, const unsigned* __restrict__ list,
                                            const unsigned* __restrict__ count,
                                            unsigned short* __restrict__ values, float k_scale, float k_offset,
                                            float k_unknown, double* __restrict__ chunk_sums, int num_chunks) {
  // launched for an upper bound of survivors when the host has not read the count yet
  if (count != nullptr && blockIdx.y >= *count) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned short v = 0;
  if (i < n) {
    const unsigned c = list[blockIdx.y];
    const int j = static_cast<int>(c / static_cast<unsigned>(R));
    const int r = static_cast<int>(c % static_cast<unsigned>(R));
    const float4 qq = rot[r];
    const Quat4 q{qq.x, qq.y, qq.z, qq.w};
    float rx, ry, rz;
    rotate_point(q, px[i], py[i], pz[i], rx, ry, rz);
    v = static_cast<unsigned short>(grid_value(g, cell_of(rx + trans[3 * j], g.resolution),
                                               cell_of(ry + trans[3 * j + 1], g.resolution),
                                               cell_of(rz + trans[3 * j + 2], g.resolution)) & 0x7FFFu);
  }
  if (i < n_stride) values[static_cast<size_t>(blockIdx.y) * n_stride + i] = v;
  if (chunk_sums != nullptr) {
    // real (double) sum of the probabilities of this wavefront's 64-point chunk: locates the binade
    // of the running sum for rtcsm_rescore_chunk_fns_kernel
    double p = 0.;
    if (i < n) p = v == 0 ? static_cast<double>(k_unknown)
                          : static_cast<double>(static_cast<float>(static_cast<int>(v)) * k_scale + k_offset);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) p += __shfl_xor(p, off, 64);
    const int chunk = i >> 6;
    if ((threadIdx.x & 63) == 0 && chunk < num_chunks) chunk_sums[static_cast<size_t>(blockIdx.y) * num_chunks + chunk] = p;
  }
}

__global__ __launch_bounds__(kScanThreads) void rtcsm_rescore_scan_kernel(
    const unsigned short* __restrict__ values, int n, int n_stride, float k_scale, float k_offset,
    float k_unknown, const unsigned* __restrict__ count, float* __restrict__ sums) {
  extern __shared__ unsigned short lds_value[];  // n_stride grid values (15 bit), input order
  if (count != nullptr && blockIdx.x >= *count) return;
  __shared__ ParityFn wave_total[kScanThreads / 64];
  __shared__ unsigned sh_m, sh_e, sh_i0, sh_cross, sh_m_before, sh_total;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    // coalesced 16-byte loads of this survivor's row (n_stride is a multiple of 8)
    const uint4* src = reinterpret_cast<const uint4*>(values + static_cast<size_t>(blockIdx.x) * n_stride);
    uint4* dst = reinterpret_cast<uint4*>(lds_value);
    for (int i = tid; i < n_stride / 8; i += kScanThreads) dst[i] = src[i];
  }
  __syncthreads();
  // probability of point i as the reference's float (probability_values.cc:27-36) ...
  auto prob = [&](int i) -> float {
    const unsigned v = lds_value[i];
    return v == 0u ? k_unknown : static_cast<float>(static_cast<int>(v)) * k_scale + k_offset;
  };
  // ... and as an exact integer in units of 2^-27 (every probability is in [2^-4, 1))
  auto fixed = [&](int i) -> unsigned {
    const unsigned b = __float_as_uint(prob(i));
    return ((b & 0x7FFFFFu) | 0x800000u) << ((b >> 23) - 123u);
  };
  if (tid == 0) {
    float s = 0.f;
    const int n0 = min(n, kSerialPrefix);
    for (int i = 0; i < n0; ++i) s += prob(i);
    const unsigned b = __float_as_uint(s);
    sh_m = (b & 0x7FFFFFu) | 0x800000u;  // s = m * 2^(e - 27), e = biased exponent - 123
    sh_e = (b >> 23) - 123u;
    sh_i0 = static_cast<unsigned>(n0);
  }
  __syncthreads();
  while (sh_i0 < static_cast<unsigned>(n)) {  // uniform: one pass per binade
    const unsigned m = sh_m, e = sh_e, i0 = sh_i0;
    const unsigned U = 1u << e, half = U >> 1, fmask = U - 1u;
    // window that must contain the crossing: every addend is >= 0.1 > 13421772 * 2^-27
    const unsigned c_min = max(13421772u >> e, 1u);
    const unsigned remaining = static_cast<unsigned>(n) - i0;
    const unsigned window = min(remaining, ((1u << 24) - m) / c_min + 2u);
    const unsigned seg = ((window + kScanThreads - 1) / kScanThreads) | 1u;  // odd: LDS banks
    const unsigned begin = i0 + static_cast<unsigned>(tid) * seg;
    const unsigned end = min(i0 + window, begin + seg);
    // phase A: this segment as a function of the incoming parity
    ParityFn f{0u, 0u, 0u, 1u};
    for (unsigned i = begin; i < end; ++i) {
      const unsigned a = fixed(static_cast<int>(i));
      const unsigned q = a >> e, fr = a & fmask;
      if (e != 0u && fr == half) {  // tie: round to even mantissa
        f.s0 += q + ((f.p0 + q) & 1u);
        f.s1 += q + ((f.p1 + q) & 1u);
        f.p0 = 0u;
        f.p1 = 0u;
      } else {
        const unsigned c = q + (fr > half ? 1u : 0u);
        f.s0 += c;
        f.s1 += c;
        f.p0 = (f.p0 + c) & 1u;
        f.p1 = (f.p1 + c) & 1u;
      }
    }
    // block-wide inclusive scan of the composition
    ParityFn inc = f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const ParityFn o = shfl_up_fn(inc, off);
      if (lane >= off) inc = compose(o, inc);
    }
    if (lane == 63) wave_total[wave] = inc;
    if (tid == 0) {
      sh_cross = 0xFFFFFFFFu;
    }
    __syncthreads();
    ParityFn before{0u, 0u, 0u, 1u};  // composition of all earlier waves
    for (int w = 0; w < wave; ++w) before = compose(before, wave_total[w]);
    ParityFn excl = shfl_up_fn(inc, 1);  // earlier lanes of this wave
    if (lane == 0) excl = ParityFn{0u, 0u, 0u, 1u};
    excl = compose(before, excl);
    const unsigned p_start = m & 1u;
    unsigned mt = m + (p_start ? excl.s1 : excl.s0);
    if (tid == kScanThreads - 1) {
      const ParityFn all = compose(before, inc);
      sh_total = p_start ? all.s1 : all.s0;
    }
    // phase B: replay the segment with the real mantissa, look for the first result >= 2^24
    unsigned my_cross = 0xFFFFFFFFu, my_before = 0u;
    for (unsigned i = begin; i < end; ++i) {
      const unsigned a = fixed(static_cast<int>(i));
      const unsigned q = a >> e, fr = a & fmask;
      unsigned c;
      if (e != 0u && fr == half) {
        c = q + ((mt + q) & 1u);
      } else {
        c = q + (fr > half ? 1u : 0u);
      }
      if (mt + c >= (1u << 24)) {
        my_cross = i;
        my_before = mt;
        break;
      }
      mt += c;
    }
    if (my_cross != 0xFFFFFFFFu) atomicMin(&sh_cross, my_cross);
    __syncthreads();
    if (my_cross != 0xFFFFFFFFu && my_cross == sh_cross) sh_m_before = my_before;
    __syncthreads();
    if (tid == 0) {
      if (sh_cross == 0xFFFFFFFFu) {  // the window ended inside this binade
        sh_m = m + sh_total;
        sh_i0 = i0 + window;
      } else {
        // exact sum of the crossing addition, rounded once to the next binade's ulp (2U)
        const unsigned long long X =
            (static_cast<unsigned long long>(sh_m_before) << e) + fixed(static_cast<int>(sh_cross));
        const unsigned e2 = e + 1u;
        const unsigned long long q2 = X >> e2, f2 = X & ((1ull << e2) - 1ull), h2 = 1ull << e;
        const unsigned long long up = (f2 > h2 || (f2 == h2 && (q2 & 1ull))) ? 1ull : 0ull;
        sh_m = static_cast<unsigned>(q2 + up);
        sh_e = e2;
        sh_i0 = sh_cross + 1u;
      }
    }
    __syncthreads();
  }
  if (tid == 0) sums[blockIdx.x] = __uint_as_float(((sh_e + 123u) << 23) | (sh_m & 0x7FFFFFu));
}

// ---- chunked variant of the exact scan (method 2) -----------------------------------------------
// The element scan above spends its time in one CU walking 64 elements per thread twice per
// binade.  Here the composition of every aligned 64-point chunk is computed ONCE, in parallel over
// the whole chip: the real (double) prefix sum tells, within a proven error bound, which binade(s)
// the reference's running float sum can be in while it crosses the chunk -- at most two -- and the
// chunk's ParityFn is stored for each.  The scan then works on chunk functions (one per thread) and
// only opens the two chunks that matter per binade: the one it resumes in and the one the sum
// leaves the binade in (both handled by a wavefront, lane per element).
constexpr int kChunk = 64;
struct ChunkFns {  // the chunk's ParityFn for up to two binades; e == 0xFFFFFFFF: absent
  unsigned e0, s00, s01, pp0;  // pp = p0 | p1 << 1
  unsigned e1, s10, s11, pp1;
};

__device__ __forceinline__ ParityFn element_fn(unsigned a, unsigned e) {
  const unsigned U = 1u << e, half = U >> 1, fmask = U - 1u;
  const unsigned q = a >> e, fr = a & fmask;
  if (e != 0u && fr == half) return ParityFn{q + (q & 1u), q + ((1u + q) & 1u), 0u, 0u};  // tie -> even
  const unsigned c = q + (fr > half ? 1u : 0u);
  return ParityFn{c, c, c & 1u, (1u + c) & 1u};
}
__device__ __forceinline__ ParityFn wave_inclusive_scan(ParityFn f, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const ParityFn o = shfl_up_fn(f, off);
    if (lane >= off) f = compose(o, f);
  }
  return f;
}
__device__ __forceinline__ unsigned fixed_of_value(unsigned v, float k_scale, float k_offset, float k_unknown) {
  const float p = v == 0u ? k_unknown : static_cast<float>(static_cast<int>(v)) * k_scale + k_offset;
  const unsigned b = __float_as_uint(p);
  return ((b & 0x7FFFFFu) | 0x800000u) << ((b >> 23) - 123u);
}
// binade index e (ulp = 2^(e-27)) of a positive real sum: floor(log2 x) + 4, never below 0
__device__ __forceinline__ int binade_of(double x) { return max(ilogb(fmax(x, 0.0625)) + 4, 0); }

__global__ __launch_bounds__(256) void rtcsm_rescore_chunk_fns_kernel(
    const unsigned short* __restrict__ values, int n, int n_stride, float k_scale, float k_offset, float k_unknown,
    const unsigned* __restrict__ count, const double* __restrict__ chunk_sums, int num_chunks,
    ChunkFns* __restrict__ fns) {
  if (count != nullptr && blockIdx.y >= *count) return;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= num_chunks) return;
  const double* sums = chunk_sums + static_cast<size_t>(blockIdx.y) * num_chunks;
  double before = 0.;
  for (int k = lane; k < c; k += 64) before += sums[k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
  const double after = before + sums[c];
  const int i = c * kChunk + lane;
  const int i_end = min(n, (c + 1) * kChunk);
  // |sequential float sum - real sum| <= sum_i 2^-24 s_i <= i 2^-24 s_i (partial sums are monotone)
  const double delta = 1.05 * static_cast<double>(i_end) * 5.9604644775390625e-8 * after + 1e-6;
  const int e_lo = binade_of(before - delta), e_hi = binade_of(after + delta);
  ChunkFns out{0xFFFFFFFFu, 0u, 0u, 0u, 0xFFFFFFFFu, 0u, 0u, 0u};
  if (e_hi - e_lo <= 1) {
    const unsigned a = i < n ? fixed_of_value(values[static_cast<size_t>(blockIdx.y) * n_stride + i], k_scale, k_offset, k_unknown) : 0u;
    const ParityFn id{0u, 0u, 0u, 1u};
    const ParityFn t0 = wave_inclusive_scan(i < n ? element_fn(a, static_cast<unsigned>(e_lo)) : id, lane);
    out.e0 = static_cast<unsigned>(e_lo);
    out.s00 = t0.s0;
    out.s01 = t0.s1;
    out.pp0 = t0.p0 | (t0.p1 << 1);
    if (e_hi != e_lo) {
      const ParityFn t1 = wave_inclusive_scan(i < n ? element_fn(a, static_cast<unsigned>(e_hi)) : id, lane);
      out.e1 = static_cast<unsigned>(e_hi);
      out.s10 = t1.s0;
      out.s11 = t1.s1;
      out.pp1 = t1.p0 | (t1.p1 << 1);
    }
  }
  if (lane == 63) fns[static_cast<size_t>(blockIdx.y) * num_chunks + c] = out;
}

// ParityFn in two words (increment in bits 0..30, parity out in bit 31): a composition is and / select / add per word,
// and the scans below move it with DPP (row shifts and the two row broadcasts) instead of ds_bpermute -- the scan
// kernel is ONE workgroup per survivor and nothing but dependent latency: ~45 wave scans and ~60 barriers a survivor
// made it 53 us for the one survivor a match usually has (round 4 profile).  Increments inside a pass's window stay
// below 2^28 (at most 2^24 / c_min elements of at most 10 c_min each), so bit 31 is free.
struct PFn2 {
  unsigned a, b;  // a: parity in 0, b: parity in 1
};
__device__ __forceinline__ PFn2 pfn2_identity() { return PFn2{0u, 0x80000000u}; }
__device__ __forceinline__ PFn2 pack_fn(const ParityFn& f) { return PFn2{f.s0 | (f.p0 << 31), f.s1 | (f.p1 << 31)}; }
__device__ __forceinline__ PFn2 compose2(const PFn2& x, const PFn2& y) {  // x first, then y
  PFn2 r;
  r.a = (x.a & 0x7FFFFFFFu) + (static_cast<int>(x.a) < 0 ? y.b : y.a);
  r.b = (x.b & 0x7FFFFFFFu) + (static_cast<int>(x.b) < 0 ? y.b : y.a);
  return r;
}
template <int kCtrl, int kRowMask>
__device__ __forceinline__ PFn2 dpp_fn(const PFn2& f) {  // lanes without a source (or outside the row mask) get the identity
  PFn2 r;
  r.a = static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(f.a), kCtrl, kRowMask, 0xf, false));
  r.b = static_cast<unsigned>(__builtin_amdgcn_update_dpp(static_cast<int>(0x80000000u), static_cast<int>(f.b), kCtrl, kRowMask, 0xf, false));
  return r;
}
__device__ __forceinline__ PFn2 wave_inclusive_scan2(PFn2 f) {
  f = compose2(dpp_fn<0x111, 0xf>(f), f);  // row_shr:1
  f = compose2(dpp_fn<0x112, 0xf>(f), f);  // row_shr:2
  f = compose2(dpp_fn<0x114, 0xf>(f), f);  // row_shr:4
  f = compose2(dpp_fn<0x118, 0xf>(f), f);  // row_shr:8
  f = compose2(dpp_fn<0x142, 0xa>(f), f);  // row_bcast:15 into rows 1 and 3
  f = compose2(dpp_fn<0x143, 0xc>(f), f);  // row_bcast:31 into rows 2 and 3
  return f;
}
__device__ __forceinline__ PFn2 wave_shift_right1(const PFn2& f) { return dpp_fn<0x138, 0xf>(f); }  // wave_shr:1, lane 0: identity
__device__ __forceinline__ PFn2 lane_of(const PFn2& f, int l) {  // l uniform
  return PFn2{static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(f.a), l)),
              static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(f.b), l))};
}
__device__ __forceinline__ unsigned apply2(const PFn2& f, unsigned parity) { return (parity ? f.b : f.a) & 0x7FFFFFFFu; }

// Thread t <-> chunk t for the whole kernel: its ChunkFns are loaded ONCE, into registers for the block's passes and into
// LDS for wave 0's walk (the file's header: chunks, super-chunks, elements).  The first 256 additions are replayed by
// wave 0 out of registers with v_readlane.  The block's pass -- the fallback -- opens the partial chunk it resumes in and
// the chunk the sum leaves the binade in by the WAVE that owns them, three barriers a pass.  Same arithmetic, same
// result bits on either path (test_sequential_sum_kernels_bit_exact and tests/test_sequential_sum_walk.py compare them
// with the element scan and the serial replay).
__global__ __launch_bounds__(kScanThreads) void rtcsm_rescore_chunk_scan_kernel(
    const unsigned short* __restrict__ values, int n, int n_stride, float k_scale, float k_offset, float k_unknown,
    const unsigned* __restrict__ count, const ChunkFns* __restrict__ fns, int num_chunks, float* __restrict__ sums,
    const unsigned* __restrict__ list, SumReadback rb) {
  if (count != nullptr && blockIdx.x >= *count) {
    if (threadIdx.x == 0) publish_sum(rb, list, false, 0.f);
    return;
  }
  __shared__ PFn2 wave_total[kScanThreads / 64];
  __shared__ unsigned sh_m, sh_e, sh_i0, sh_cross_t, sh_total, sh_mismatch_t, sh_force_serial;
  // every chunk's functions for wave 0's walk: {e0's PFn2, e1's PFn2} and e0 | e1 << 8 (0xFF: absent; a binade is < 32)
  __shared__ uint4 lds_fn[kScanThreads];
  __shared__ unsigned lds_fn_e[kScanThreads];
  // super-chunk w = the 64 chunks of wave w: its function for the (at most two) binades that ALL of its chunks carry
  __shared__ unsigned super_e[kScanThreads / 64][2];
  __shared__ PFn2 super_fn[kScanThreads / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ChunkFns none{0xFFFFFFFFu, 0u, 0u, 0u, 0xFFFFFFFFu, 0u, 0u, 0u};
  const ChunkFns cf = tid < num_chunks ? fns[static_cast<size_t>(blockIdx.x) * num_chunks + tid] : none;  // in flight during the copy
  // The values stay in global memory: the walk opens two or three chunks a pass, and reading those 128 bytes from L2
  // is cheaper than copying up to 128 KB into LDS first (measured at 65 536 points: 25.4 -> 23.2 us a survivor).
  const unsigned short* __restrict__ vals = values + static_cast<size_t>(blockIdx.x) * n_stride;
  {
    const PFn2 cf0{cf.s00 | ((cf.pp0 & 1u) << 31), cf.s01 | ((cf.pp0 >> 1) << 31)};
    const PFn2 cf1{cf.s10 | ((cf.pp1 & 1u) << 31), cf.s11 | ((cf.pp1 >> 1) << 31)};
    lds_fn[tid] = make_uint4(cf0.a, cf0.b, cf1.a, cf1.b);
    lds_fn_e[tid] = (cf.e0 & 0xFFu) | ((cf.e1 & 0xFFu) << 8);
    // a binade that all 64 chunks carry is one of the first chunk's two (all sixteen waves are whole here: the scans are DPP)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned E = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(k == 0 ? cf.e0 : cf.e1), 0));
      const bool has0 = cf.e0 == E, has = E != 0xFFFFFFFFu && (has0 || cf.e1 == E);
      const PFn2 total = lane_of(wave_inclusive_scan2(has ? (has0 ? cf0 : cf1) : pfn2_identity()), 63);
      const bool all = __ballot(has) == ~0ull;
      if (lane == 0) {
        super_e[wave][k] = all ? E : 0xFFFFFFFFu;
        super_fn[wave][k] = total;
      }
    }
  }
  __syncthreads();
  auto prob = [&](unsigned v) { return v == 0u ? k_unknown : static_cast<float>(static_cast<int>(v)) * k_scale + k_offset; };
  auto fixed = [&](unsigned i) { return fixed_of_value(vals[i], k_scale, k_offset, k_unknown); };
  const int n0 = min(n, kSerialPrefix);
  if (wave == 0) {
    float s = 0.f;
    if (n0 == kSerialPrefix) {
      // element k * 64 + l sits in lane l's register k: the 256 sequential additions read them with v_readlane
      float pv[kSerialPrefix / 64];
#pragma unroll
      for (int k = 0; k < kSerialPrefix / 64; ++k) pv[k] = prob(vals[k * 64 + lane]);
#pragma unroll
      for (int k = 0; k < kSerialPrefix / 64; ++k)
#pragma unroll
        for (int l = 0; l < 64; ++l) s += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pv[k]), l));
    } else {
      for (int i = 0; i < n0; ++i) s += prob(vals[i]);
    }
    // ---- every binade by wave 0 ALONE.  The sum doubles from binade to binade, so the early passes cover a few dozen
    // chunks each and the last ones tens of thousands of additions -- and a block pass costs three barriers of sixteen
    // waves and a serial compose over the wave totals whatever its window (4.4 us a pass).  One step of the loop below
    // opens up to 64 chunks from the one the walk resumes in (lane l <-> chunk c0 + l, functions out of LDS), up to the
    // window's end or, if that is further, up to the next super-chunk boundary; from a boundary it skips whole
    // super-chunks (lane s <-> super-chunk s) up to the first that crosses, has no function for the binade or is cut by
    // the window's end, which the next step opens.  Every step leaves an exact (m, e, i0) further on, so a pass is a few
    // steps of wave-uniform state.  A chunk without a function in front of the crossing leaves the pass to the block.
    const unsigned b0 = __float_as_uint(s);
    unsigned m = (b0 & 0x7FFFFFu) | 0x800000u, e = (b0 >> 23) - 123u, i0 = static_cast<unsigned>(n0);
    const PFn2 idw = pfn2_identity();
    while (i0 < static_cast<unsigned>(n)) {
      const unsigned c_min = max(13421772u >> e, 1u);
      const unsigned window = min(static_cast<unsigned>(n) - i0, ((1u << 24) - m) / c_min + 2u);
      const unsigned c0 = i0 / kChunk;
      const unsigned i_lim = min(static_cast<unsigned>(n), ((i0 + window + kChunk - 1u) / kChunk) * kChunk);
      const unsigned last_chunk = (i_lim - 1u) / kChunk;
      // chunks [c0, cend) in this step: the window's rest if 64 lanes reach it, else up to the super-chunk boundary
      const unsigned cend = last_chunk - c0 < 64u ? last_chunk + 1u : ((c0 >> 6) + 1u) << 6;
      const unsigned c = c0 + static_cast<unsigned>(lane);
      const unsigned begin = max(i0, c * kChunk), end = min(i_lim, (c + 1u) * kChunk);
      const bool in_window = c < cend;  // <= last_chunk < num_chunks
      const bool resume_partial = (i0 & (kChunk - 1u)) != 0u;
      PFn2 f = idw;
      bool mismatch = false;
      if (in_window && !(resume_partial && lane == 0)) {
        const unsigned ce = lds_fn_e[c];
        const uint4 cw = lds_fn[c];
        if ((ce & 0xFFu) == e) f = PFn2{cw.x, cw.y};
        else if ((ce >> 8) == e) f = PFn2{cw.z, cw.w};
        else mismatch = true;
      }
      if (resume_partial) {  // the chunk the walk resumes in is partial: lane per element
        const unsigned he = min(i_lim, (c0 + 1u) * kChunk);
        const unsigned i = i0 + static_cast<unsigned>(lane);
        const PFn2 h = wave_inclusive_scan2(i < he ? pack_fn(element_fn(fixed(i), e)) : idw);
        const PFn2 whole = lane_of(h, 63);
        if (lane == 0) f = whole;
      }
      const PFn2 inc = wave_inclusive_scan2(f);
      const PFn2 excl = wave_shift_right1(inc);
      const unsigned p_start = m & 1u;
      const unsigned mt_start = m + apply2(excl, p_start), mt_end = m + apply2(inc, p_start);
      const unsigned long long cross_mask = __ballot(in_window && mt_end >= (1u << 24) && mt_start < (1u << 24));
      const unsigned long long mism_mask = __ballot(mismatch);
      const int cross_l = cross_mask != 0ull ? __ffsll(static_cast<long long>(cross_mask)) - 1 : 64;
      const int mism_l = mism_mask != 0ull ? __ffsll(static_cast<long long>(mism_mask)) - 1 : 64;
      if (mism_l < cross_l || (cross_l == 64 && mism_l != 64)) break;  // the block's pass knows how to open such chunks
      if (cross_l == 64) {  // no crossing in these chunks (lanes behind cend are the identity)
        m = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(mt_end), 63));
        i0 = min(i_lim, cend * kChunk);
        if (i0 >= i_lim) continue;  // the cloud ended inside this binade
        // at a super-chunk boundary with window left: skip whole super-chunks.  One that the window's end cuts, one without
        // a function for this binade and one the sum leaves the binade in halt the skip; the next step opens it.
        const unsigned s_first = cend >> 6, s_last = last_chunk >> 6;
        const bool whole_last = (last_chunk & 63u) == 63u;
        const unsigned sc = static_cast<unsigned>(lane);
        const bool active = sc >= s_first && sc <= s_last;  // s_last < kScanThreads / 64
        PFn2 g = idw;
        bool stop = active;
        if (active && (sc < s_last || whole_last)) {
          if (super_e[sc][0] == e) {
            g = super_fn[sc][0];
            stop = false;
          } else if (super_e[sc][1] == e) {
            g = super_fn[sc][1];
            stop = false;
          }
        }
        const PFn2 ginc = wave_inclusive_scan2(g);
        const PFn2 gexc = wave_shift_right1(ginc);
        const unsigned gp = m & 1u;
        const unsigned g_start = m + apply2(gexc, gp), g_end = m + apply2(ginc, gp);
        const unsigned long long halt_mask = __ballot(active && (stop || g_end >= (1u << 24)));
        const int halt = halt_mask != 0ull ? __ffsll(static_cast<long long>(halt_mask)) - 1 : static_cast<int>(s_last) + 1;
        m = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(g_start), halt));  // lane s_last + 1: the identity
        i0 = min(i_lim, static_cast<unsigned>(halt) * (64u * kChunk));
        continue;
      }
      const unsigned cb = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(begin), cross_l));
      const unsigned ce = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(end), cross_l));
      const unsigned ms = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(mt_start), cross_l));
      const unsigned i = cb + static_cast<unsigned>(lane);
      const unsigned a_i = i < ce ? fixed(i) : 0u;
      const PFn2 sc = wave_inclusive_scan2(i < ce ? pack_fn(element_fn(a_i, e)) : idw);
      const PFn2 ex = wave_shift_right1(sc);
      const unsigned ps = ms & 1u;
      const unsigned m_before = ms + apply2(ex, ps), m_after = ms + apply2(sc, ps);
      const unsigned long long crossed = __ballot(i < ce && m_after >= (1u << 24));
      if (crossed == 0ull) break;  // (cannot happen: the chunk's function said it crosses) -- the block decides
      const int first = __ffsll(static_cast<long long>(crossed)) - 1;
      const unsigned mb = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(m_before), first));
      const unsigned af = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(a_i), first));
      // exact sum of the crossing addition, rounded once to the next binade's ulp (2U)
      const unsigned long long X = (static_cast<unsigned long long>(mb) << e) + af;
      const unsigned e2 = e + 1u;
      const unsigned long long q2 = X >> e2, f2 = X & ((1ull << e2) - 1ull), h2 = 1ull << e;
      const unsigned long long up = (f2 > h2 || (f2 == h2 && (q2 & 1ull))) ? 1ull : 0ull;
      m = static_cast<unsigned>(q2 + up);
      e = e2;
      i0 = cb + static_cast<unsigned>(first) + 1u;
    }
    if (lane == 0) {
      sh_m = m;
      sh_e = e;
      sh_i0 = i0;
      sh_force_serial = 0u;
    }
  }
  __syncthreads();
  const PFn2 id = pfn2_identity();
  while (sh_i0 < static_cast<unsigned>(n)) {  // uniform: one pass per binade
    const unsigned m = sh_m, e = sh_e, i0 = sh_i0, force_serial = sh_force_serial;
    // window that must contain the crossing (every addend >= 0.1 > 13421772 * 2^-27), rounded up to
    // a chunk boundary: elements behind the crossing are never looked at
    const unsigned c_min = max(13421772u >> e, 1u);
    const unsigned remaining = static_cast<unsigned>(n) - i0;
    const unsigned window = min(remaining, ((1u << 24) - m) / c_min + 2u);
    const unsigned c0 = i0 / kChunk;
    const unsigned i_lim = min(static_cast<unsigned>(n), ((i0 + window + kChunk - 1u) / kChunk) * kChunk);
    // thread t <-> chunk t, clipped to [i0, i_lim): chunks before the one the walk resumes in and behind the window
    // are the identity
    const unsigned c = static_cast<unsigned>(tid);
    const unsigned begin = max(i0, c * kChunk), end = min(i_lim, (c + 1u) * kChunk);
    const bool in_window = begin < end && c >= c0;
    PFn2 f = id;
    bool mismatch = false;
    if (in_window && c != c0) {
      if (cf.e0 == e) f = PFn2{cf.s00 | ((cf.pp0 & 1u) << 31), cf.s01 | ((cf.pp0 >> 1) << 31)};
      else if (cf.e1 == e) f = PFn2{cf.s10 | ((cf.pp1 & 1u) << 31), cf.s11 | ((cf.pp1 >> 1) << 31)};
      else mismatch = true;
    }
    // A chunk without a function for this binade lies BEHIND the crossing (the window bound is loose
    // by up to 9x, and the real prefix proves the sum has left the binade by then): it stays the
    // identity and is never selected.  Should one ever sit before the crossing -- a violated bound --
    // the pass is repeated with such chunks opened element by element (sh_force_serial).
    if (mismatch && force_serial) {
      ParityFn g = ParityFn{0u, 0u, 0u, 1u};
      for (unsigned i = begin; i < end; ++i) g = compose(g, element_fn(fixed(i), e));
      f = pack_fn(g);
      mismatch = false;
    }
    if (static_cast<unsigned>(wave) == (c0 >> 6)) {  // the chunk the walk resumes in is partial: lane per element, by its wave
      const unsigned he = min(i_lim, (c0 + 1u) * kChunk);
      const unsigned i = i0 + static_cast<unsigned>(lane);
      const PFn2 h = wave_inclusive_scan2(i < he ? pack_fn(element_fn(fixed(i), e)) : id);
      const PFn2 whole = lane_of(h, 63);
      if (static_cast<unsigned>(lane) == (c0 & 63u)) f = whole;
    }
    // block-wide inclusive scan over the chunk functions
    const PFn2 inc = wave_inclusive_scan2(f);
    if (lane == 63) wave_total[wave] = inc;
    if (tid == 0) {
      sh_cross_t = 0xFFFFFFFFu;
      sh_mismatch_t = 0xFFFFFFFFu;
    }
    __syncthreads();  // (1) wave totals, reset words
    if (mismatch) atomicMin(&sh_mismatch_t, static_cast<unsigned>(tid));
    PFn2 before = id;
    for (int w = 0; w < wave; ++w) before = compose2(before, wave_total[w]);
    const PFn2 excl = compose2(before, wave_shift_right1(inc));
    const PFn2 incl = compose2(before, inc);
    const unsigned p_start = m & 1u;
    const unsigned mt_start = m + apply2(excl, p_start);
    const unsigned mt_end = m + apply2(incl, p_start);
    if (tid == kScanThreads - 1) sh_total = mt_end - m;
    const bool crosses = in_window && mt_end >= (1u << 24) && mt_start < (1u << 24);
    if (crosses) atomicMin(&sh_cross_t, static_cast<unsigned>(tid));
    __syncthreads();  // (2) first crossing chunk, first chunk without a function, total
    const unsigned cross_t = sh_cross_t, mismatch_t = sh_mismatch_t;
    if (mismatch_t < cross_t || (cross_t == 0xFFFFFFFFu && mismatch_t != 0xFFFFFFFFu)) {
      __syncthreads();  // everyone has read the verdict
      if (tid == 0) sh_force_serial = 1u;
      __syncthreads();
      continue;  // same (m, e, i0), chunks without a function opened serially
    }
    if (cross_t == 0xFFFFFFFFu) {
      if (tid == 0) {  // the cloud ended inside this binade
        sh_m = m + sh_total;
        sh_i0 = i_lim;
      }
    } else if (static_cast<unsigned>(wave) == (cross_t >> 6)) {  // open the crossing chunk: lane per element, by its wave
      const int cl = static_cast<int>(cross_t & 63u);
      const unsigned cb = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(begin), cl));
      const unsigned ce = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(end), cl));
      const unsigned ms = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(mt_start), cl));
      const unsigned i = cb + static_cast<unsigned>(lane);
      const PFn2 sc = wave_inclusive_scan2(i < ce ? pack_fn(element_fn(fixed(i), e)) : id);
      const PFn2 ex = wave_shift_right1(sc);
      const unsigned ps = ms & 1u;
      const unsigned m_before = ms + apply2(ex, ps);
      const unsigned m_after = ms + apply2(sc, ps);
      const unsigned long long crossed = __ballot(i < ce && m_after >= (1u << 24));
      const int first = __ffsll(static_cast<long long>(crossed)) - 1;
      if (lane == first) {
        // exact sum of the crossing addition, rounded once to the next binade's ulp (2U)
        const unsigned long long X = (static_cast<unsigned long long>(m_before) << e) + fixed(i);
        const unsigned e2 = e + 1u;
        const unsigned long long q2 = X >> e2, f2 = X & ((1ull << e2) - 1ull), h2 = 1ull << e;
        const unsigned long long up = (f2 > h2 || (f2 == h2 && (q2 & 1ull))) ? 1ull : 0ull;
        sh_m = static_cast<unsigned>(q2 + up);
        sh_e = e2;
        sh_i0 = i + 1u;
      }
    }
    __syncthreads();  // (3) the next pass's state
  }
  if (tid == 0) {
    const float sum = __uint_as_float(((sh_e + 123u) << 23) | (sh_m & 0x7FFFFFu));
    sums[blockIdx.x] = sum;
    publish_sum(rb, list, true, sum);
  }
}

// ---------------------------------------------------------------------------------- host side
// The library's rescoring method (the chunk scan), and the cloud size up to which a match replays the sum serially
// instead: for small clouds (the reference's ~170 filtered points) the serial replay is one launch of ~5 us, the chunk
// scan three.  All methods return identical bits (test_sequential_sum_kernels_bit_exact).
constexpr int kRescoreMethod = 2;
constexpr int64_t kRescoreSerialMaxPoints = 1024;

int sequential_sum_method(int64_t num_points) { return num_points <= kRescoreSerialMaxPoints ? 0 : kRescoreMethod; }

// Scratch of methods 1 and 2 for `count` candidates of n points: [values | chunk sums | chunk functions]
struct ScratchLayout {
  size_t sums_at, fns_at, bytes;
};
static ScratchLayout scratch_layout(size_t count, int n) {
  const int n_stride = (n + 7) & ~7, num_chunks = (n + kChunk - 1) / kChunk;
  const size_t values_bytes = align256(count * n_stride * 2), sums_bytes = align256(count * num_chunks * 8);
  return {values_bytes, values_bytes + sums_bytes, values_bytes + sums_bytes + count * num_chunks * sizeof(ChunkFns)};
}

int launch_sequential_sums(dliom_ctx* ctx, int method, const GridView& gv, const dliom_cloud& cloud, const float4* d_rot,
                           int R, const float* d_trans, const unsigned* d_list, const unsigned* d_count, unsigned count,
                           DevBuf* scratch, float* d_ksums, const SumReadback* readback) {
  const SumReadback rb = readback != nullptr ? *readback : SumReadback{};
  const float k_scale = kValueToProbabilityScale, k_offset = kValueToProbabilityOffset, k_unknown = kUnknownProbability;
  const int n = static_cast<int>(cloud.n);
  const int n_stride = (n + 7) & ~7;
  const size_t scan_lds = static_cast<size_t>(n_stride) * 2;
  // method 1 holds a candidate's values in LDS and method 2 a chunk per thread: 65 536 points at most for either
  if (method == 0 || scan_lds > 128 * 1024 || count > 65535) {
    hipLaunchKernelGGL(rtcsm_rescore_kernel, dim3(count), dim3(256), 0, ctx->stream, gv, cloud.d_x, cloud.d_y, cloud.d_z, n,
                       d_rot, R, d_trans, d_list, d_count, k_scale, k_offset, k_unknown, d_ksums, rb);
    DLIOM_HIP_TRY(hipGetLastError());
    return DLIOM_OK;
  }
  const int num_chunks = (n + kChunk - 1) / kChunk;
  const ScratchLayout at = scratch_layout(count, n);
  DLIOM_TRY(scratch->reserve(at.bytes));
  char* base = static_cast<char*>(scratch->p);
  unsigned short* d_values = reinterpret_cast<unsigned short*>(base);
  double* d_chunk_sums = method == 2 ? reinterpret_cast<double*>(base + at.sums_at) : nullptr;
  ChunkFns* d_fns = reinterpret_cast<ChunkFns*>(base + at.fns_at);
  hipLaunchKernelGGL(rtcsm_rescore_values_kernel, dim3((n_stride + 255) / 256, count), dim3(256), 0, ctx->stream, gv,
                     cloud.d_x, cloud.d_y, cloud.d_z, n, n_stride, d_rot, R, d_trans, d_list, d_count, d_values, k_scale,
                     k_offset, k_unknown, d_chunk_sums, num_chunks);
  if (method == 2) {
    hipLaunchKernelGGL(rtcsm_rescore_chunk_fns_kernel, dim3((num_chunks + 3) / 4, count), dim3(256), 0, ctx->stream, d_values,
                       n, n_stride, k_scale, k_offset, k_unknown, d_count, d_chunk_sums, num_chunks, d_fns);
    hipLaunchKernelGGL(rtcsm_rescore_chunk_scan_kernel, dim3(count), dim3(kScanThreads), 0, ctx->stream, d_values, n,
                       n_stride, k_scale, k_offset, k_unknown, d_count, d_fns, num_chunks, d_ksums, d_list, rb);
  } else {
    hipLaunchKernelGGL(rtcsm_rescore_scan_kernel, dim3(count), dim3(kScanThreads), scan_lds, ctx->stream, d_values, n, n_stride,
                       k_scale, k_offset, k_unknown, d_count, d_ksums);
  }
  DLIOM_HIP_TRY(hipGetLastError());
  return DLIOM_OK;
}

// Sequential float sums, in point order, of the LUT probabilities of `cloud` under k explicit float
// poses: sums[i] = sum_p P(value(cell(q_i * p + t_i))) accumulated like `score += p`
// (low_resolution_matcher.cc:27-34; the same loop as rtcsm_3d.cc:101-104).  Uses ctx->bounds,
// ctx->rescore and ctx->misc as scratch; synchronises the stream.
int sequential_probability_sums(dliom_ctx* ctx, const dliom_cloud& cloud, const dliom_grid* grid, const float* poses7,
                                int k, float* sums) {
  if (k <= 0 || k > 65535 || cloud.n <= 0) return DLIOM_ERR_INVALID_ARGUMENT;
  const size_t K = static_cast<size_t>(k);
  const size_t rot_bytes = align256(K * 16), trans_bytes = align256(K * 12), list_bytes = align256(K * 4);
  DLIOM_TRY(ctx->bounds.reserve(rot_bytes + trans_bytes + list_bytes));
  std::vector<char> host(rot_bytes + trans_bytes + list_bytes, 0);
  float* hr = reinterpret_cast<float*>(host.data());
  float* ht = reinterpret_cast<float*>(host.data() + rot_bytes);
  unsigned* hl = reinterpret_cast<unsigned*>(host.data() + rot_bytes + trans_bytes);
  for (size_t i = 0; i < K; ++i) {
    const float* p = poses7 + 7 * i;
    hr[4 * i] = p[3];
    hr[4 * i + 1] = p[4];
    hr[4 * i + 2] = p[5];
    hr[4 * i + 3] = p[6];
    ht[3 * i] = p[0];
    ht[3 * i + 1] = p[1];
    ht[3 * i + 2] = p[2];
    hl[i] = static_cast<unsigned>(i * K + i);  // the kernels decode c -> (translation c / R, rotation c % R), R = k
  }
  char* base = static_cast<char*>(ctx->bounds.p);
  DLIOM_HIP_TRY(hipMemcpyAsync(base, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
  const float4* d_rot = reinterpret_cast<const float4*>(base);
  const float* d_trans = reinterpret_cast<const float*>(base + rot_bytes);
  const unsigned* d_list = reinterpret_cast<const unsigned*>(base + rot_bytes + trans_bytes);
  DLIOM_TRY(ctx->rescore.reserve(list_bytes));
  float* d_ksums = ctx->rescore.as<float>();
  DLIOM_TRY(launch_sequential_sums(ctx, kRescoreMethod, grid->view(), cloud, d_rot, k, d_trans, d_list, nullptr,
                                   static_cast<unsigned>(k), &ctx->misc, d_ksums));
  if (K <= 1024) {  // a few sums (the loop-closure matcher asks for one at a time): packed by a kernel, polled
    const GatherJob job{d_ksums, static_cast<unsigned>(K)};
    static_assert(1024 * 4 <= kPinSequentialSums.bytes, "the sums fit their region");
    float* h = pinned_at<float>(ctx, kPinSequentialSums);
    DLIOM_TRY(gather_and_wait(ctx, &job, 1, h));  // also keeps `host` alive long enough: the upload is in front of it
    std::memcpy(sums, h, K * 4);
    return DLIOM_OK;
  }
  DLIOM_HIP_TRY(hipMemcpyAsync(sums, d_ksums, K * 4, hipMemcpyDeviceToHost, ctx->stream));
  DLIOM_HIP_TRY(hipStreamSynchronize(ctx->stream));  // also keeps `host` alive long enough
  ++ctx->host_syncs;
  return DLIOM_OK;
}

int sequential_probability_sums_enqueue(dliom_ctx* ctx, const SequentialSumJob* jobs, int num_jobs, const float4* d_rot,
                                        const float* d_trans, const unsigned* d_list, float* d_sums) {
  // launch_sequential_sums' scratch, reserved once for the largest job: growing it between the launches would free
  // memory the launches before still use
  size_t most = 0;
  for (int j = 0; j < num_jobs; ++j) {
    if (jobs[j].k <= 0 || jobs[j].k > 65535 || jobs[j].cloud->n <= 0) return DLIOM_ERR_INVALID_ARGUMENT;
    most = std::max(most, scratch_layout(static_cast<size_t>(jobs[j].k), static_cast<int>(jobs[j].cloud->n)).bytes);
  }
  DLIOM_TRY(ctx->misc.reserve(most));
  for (int j = 0; j < num_jobs; ++j) {
    const SequentialSumJob& b = jobs[j];
    DLIOM_TRY(launch_sequential_sums(ctx, kRescoreMethod, b.grid->view(), *b.cloud, d_rot + b.first, b.k, d_trans + 3 * b.first,
                                     d_list + b.first, nullptr, static_cast<unsigned>(b.k), &ctx->misc, d_sums + b.first));
  }
  return DLIOM_OK;
}

}  // namespace dliom
