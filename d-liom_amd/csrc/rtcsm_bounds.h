// The rounding-error bound of the reference's sequential float sum that rtcsm_bounds_kernel widens a candidate's score
// interval by, as a loop and as the per-match table the kernel looks it up in.  Plain C++ on the host (rtcsm3d.hip,
// tests/cpp/rtcsm_bound_table_check.cc); the table look-up also on the device.
#ifndef DLIOM_CSRC_RTCSM_BOUNDS_H_
#define DLIOM_CSRC_RTCSM_BOUNDS_H_

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DLIOM_BOUNDS_HD __host__ __device__
#else
#define DLIOM_BOUNDS_HD
#endif

namespace dliom {

// Upper bound of the accumulated rounding error of the reference's sequential float sum.
// Each addition is off by at most half an ulp of its result (round to nearest) and the partial
// sums s_m are monotone, so the error after m additions is <= m 2^-24 s_m; with every addend
// <= 0.9000001 this gives s_m <= 0.9000001 m / (1 - m 2^-24) <= 0.93 m for m <= 2^19.  Together
// with s_m <= U (the final sum's upper bound) the (i+1)-th result is <= min(0.93 (i+1), U).
DLIOM_BOUNDS_HD inline double seq_sum_error_bound(int n, double U) {
  double err = 0.0;
  long long i = 0;  // indices [0, i) are already accounted for
  // binade k: results in [2^k, 2^(k+1)) have ulp 2^(k-23).  Index i (the (i+1)-th addition) has
  // its result bounded by B_i = min(0.93 (i+1), U).
  for (int k = -4; k < 64 && i < n; ++k) {
    const double top = ldexp(1.0, k + 1);
    long long last;  // indices [i, last) are charged this binade's ulp
    if (U < top) {
      last = n;  // the cap keeps every remaining result below `top`
    } else {
      // 0.93 (idx+1) < top  <=>  idx + 1 < top / 0.93 ; one index fewer guards the division's rounding
      last = static_cast<long long>(floor(top / 0.93)) - 1;
      if (last > n) last = n;
    }
    if (last > i) {
      err += 0.5 * ldexp(1.0, k - 23) * static_cast<double>(last - i);
      i = last;
    }
  }
  return err;
}

// The loop looks at U only in `U < 2^(k+1)`, k = -4 .. 63: for U in [2^K, 2^(K+1)) it charges the binades below K in
// full and binade K with the remaining indices, whatever U is inside the binade.  So the bound is a function of n and
// of K = floor(log2 U) clamped to [-4, 63] (a U below 2^-4 behaves like binade -4; a U of 2^64 or more, or a NaN, fails
// every comparison like binade 63 does for the n <= 2^19 the bound is used for): one table of 68 doubles a match.
constexpr int kSeqSumBoundFirstBinade = -4;
constexpr int kSeqSumBoundBinades = 68;
struct SeqSumBoundTable {
  double err[kSeqSumBoundBinades];  // err[K + 4] = seq_sum_error_bound(n, 2^K)
};
inline void fill_seq_sum_bound_table(int n, SeqSumBoundTable* t) {
  for (int K = 0; K < kSeqSumBoundBinades; ++K) t->err[K] = seq_sum_error_bound(n, ldexp(1.0, K + kSeqSumBoundFirstBinade));
}
// index of U's binade in the table, from the double's exponent field (zero and denormals: far below 2^-4)
DLIOM_BOUNDS_HD inline int seq_sum_bound_index(double U) {
  if (!(U > 0.0)) return U == U ? 0 : kSeqSumBoundBinades - 1;  // zero, negative: below every `top`; NaN: below none
  uint64_t bits;
  memcpy(&bits, &U, 8);
  const int K = static_cast<int>((bits >> 52) & 0x7ffu) - 1023;
  const int idx = K - kSeqSumBoundFirstBinade;
  return idx < 0 ? 0 : (idx >= kSeqSumBoundBinades ? kSeqSumBoundBinades - 1 : idx);
}

}  // namespace dliom

#endif  // DLIOM_CSRC_RTCSM_BOUNDS_H_
