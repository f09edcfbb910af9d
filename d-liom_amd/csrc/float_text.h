// The text of one float as XyzWriterPointsProcessor writes it (dliom.h "XYZ text of export batches"; DESIGN.md section
// 3.29): std::ostream << std::setprecision(6) << float, which under glibc / libstdc++ is printf("%.6g") of the promoted
// value.  One formatter for the host (dliom_float_text) and the device (points_text.hip): no HIP runtime call, no
// floating-point operation at all -- every digit comes from integer arithmetic on the float's bits -- and no array that
// a lane would index with a variable, so the device keeps everything in registers.
//
// The arithmetic.  A finite non-zero |value| is v = m * 2^e with m < 2^24, -149 <= e <= 104, and L = floor(log2 v) is
// e + (index of m's highest bit).  The decimal exponent is estimated as X0 = floor(L * 1233 / 4096) (1233 / 4096 is just
// below log10 2): never above floor(log10 v), at most one below it.  With s = 5 - X0,
//     Q = floor(num / den),  rem = num - Q * den,
//     num = m * 5^max(s, 0) * 2^max(e + s, 0),   den = 5^max(-s, 0) * 2^max(-e - s, 0),
// so Q = floor(v * 10^s) lies in [10^5, 10^7).
//   Q < 10^6  : X = X0, the six digits are D = Q and the discarded fraction is rem / den: compared with 1/2 as
//               2 * rem against den.
//   Q >= 10^6 : the estimate was one short.  X = X0 + 1, D = floor(Q / 10), and the discarded fraction is
//               ((Q mod 10) + rem / den) / 10: above, below or at 1/2 by (Q mod 10) against 5, then rem against 0.  (The
//               same D, X and decision as dividing again with s - 1, without the second division.)
// D is rounded to nearest, ties to even; D = 10^6 after rounding up becomes 10^5 with X + 1.
//
// Widths.  Common path, -8 <= X0 <= 18 (1e-8 <= v < 1e19; every fixed-notation value is in it): 5^|s| < 2^31, num <
// 2^63 and den < 2^62 -- 64-bit words; for s >= 0 den is a power of two and the division is a shift.  Every other
// value takes the multiword path on five 32-bit limbs: num < 2^130, den < 2^108, and the long division's shifted
// divisor den * 2^24 < 2^132 of the 160 bits.  tests/cpp/float_text_check.cc compiles this header with
// DLIOM_FLOAT_TEXT_CHECK, which turns each of these bounds (and 10^5 <= Q < 10^7) into an assertion, and runs all 2^32
// bit patterns (profiles/float_text_exhaustive.txt).
#ifndef DLIOM_CSRC_FLOAT_TEXT_H_
#define DLIOM_CSRC_FLOAT_TEXT_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DLIOM_FT_HD __host__ __device__ __forceinline__
#else
#define DLIOM_FT_HD inline
#endif

#ifdef DLIOM_FLOAT_TEXT_CHECK
#include <cstdio>
#include <cstdlib>
#define DLIOM_FT_ASSERT(cond, bits)                                                       \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      std::fprintf(stderr, "float_text.h: %s fails for bits 0x%08x\n", #cond, (bits));    \
      std::abort();                                                                       \
    }                                                                                     \
  } while (0)
#else
#define DLIOM_FT_ASSERT(cond, bits) ((void)0)
#endif

namespace dliom {

constexpr int kFloatTextMax = 12;  // "-0.000123456", "-1.17549e-38"

// The characters, first one in the low byte of `lo`; characters 8 to 11 in `hi`.
struct FloatText {
  uint64_t lo;
  uint32_t hi;
  int length;
};

DLIOM_FT_HD void ft_put(FloatText& t, unsigned c) {
  const unsigned at = static_cast<unsigned>(t.length);
  t.lo |= at < 8u ? static_cast<uint64_t>(c) << (8u * (at & 7u)) : uint64_t{0};
  t.hi |= at >= 8u ? c << (8u * (at & 3u)) : 0u;
  ++t.length;
}
DLIOM_FT_HD unsigned ft_char(const FloatText& t, int i) {
  return static_cast<unsigned>(i < 8 ? t.lo >> (8 * i) : static_cast<uint64_t>(t.hi) >> (8 * (i - 8))) & 0xffu;
}

// 5^k for k <= 13 (5^13 < 2^31), by selection: a table in memory would be a load a lane
DLIOM_FT_HD uint32_t ft_pow5(int k) {
  uint32_t p = 1u;
  for (int i = 0; i < 13; ++i) p = i < k ? p * 5u : p;
  return p;
}

// ---- the multiword path: 160-bit unsigned numbers, limb 0 least significant -------------------------------------------
struct FtWide {
  uint32_t w0, w1, w2, w3, w4;
};
DLIOM_FT_HD void ft_mul_small(FtWide& a, uint32_t f) {
  uint64_t c = static_cast<uint64_t>(a.w0) * f;
  a.w0 = static_cast<uint32_t>(c);
  c = static_cast<uint64_t>(a.w1) * f + (c >> 32);
  a.w1 = static_cast<uint32_t>(c);
  c = static_cast<uint64_t>(a.w2) * f + (c >> 32);
  a.w2 = static_cast<uint32_t>(c);
  c = static_cast<uint64_t>(a.w3) * f + (c >> 32);
  a.w3 = static_cast<uint32_t>(c);
  c = static_cast<uint64_t>(a.w4) * f + (c >> 32);
  a.w4 = static_cast<uint32_t>(c);
}
// a *= 5^p5 * 2^p2
DLIOM_FT_HD void ft_scale(FtWide& a, int p5, int p2) {
  while (p5 > 0) {
    const int k = p5 < 13 ? p5 : 13;
    ft_mul_small(a, ft_pow5(k));
    p5 -= k;
  }
  while (p2 > 0) {
    const int k = p2 < 31 ? p2 : 31;
    ft_mul_small(a, 1u << k);
    p2 -= k;
  }
}
DLIOM_FT_HD void ft_shr1(FtWide& a) {
  a.w0 = (a.w0 >> 1) | (a.w1 << 31);
  a.w1 = (a.w1 >> 1) | (a.w2 << 31);
  a.w2 = (a.w2 >> 1) | (a.w3 << 31);
  a.w3 = (a.w3 >> 1) | (a.w4 << 31);
  a.w4 >>= 1;
}
DLIOM_FT_HD bool ft_ge(const FtWide& a, const FtWide& b) {
  if (a.w4 != b.w4) return a.w4 > b.w4;
  if (a.w3 != b.w3) return a.w3 > b.w3;
  if (a.w2 != b.w2) return a.w2 > b.w2;
  if (a.w1 != b.w1) return a.w1 > b.w1;
  return a.w0 >= b.w0;
}
DLIOM_FT_HD bool ft_equal(const FtWide& a, const FtWide& b) {
  return a.w0 == b.w0 && a.w1 == b.w1 && a.w2 == b.w2 && a.w3 == b.w3 && a.w4 == b.w4;
}
DLIOM_FT_HD void ft_sub(FtWide& a, const FtWide& b) {  // a >= b
  uint64_t d = static_cast<uint64_t>(a.w0) - b.w0;
  a.w0 = static_cast<uint32_t>(d);
  d = static_cast<uint64_t>(a.w1) - b.w1 - ((d >> 32) & 1u);
  a.w1 = static_cast<uint32_t>(d);
  d = static_cast<uint64_t>(a.w2) - b.w2 - ((d >> 32) & 1u);
  a.w2 = static_cast<uint32_t>(d);
  d = static_cast<uint64_t>(a.w3) - b.w3 - ((d >> 32) & 1u);
  a.w3 = static_cast<uint32_t>(d);
  d = static_cast<uint64_t>(a.w4) - b.w4 - ((d >> 32) & 1u);
  a.w4 = static_cast<uint32_t>(d);
}

// Q = floor(v * 10^s) and how the discarded fraction rem / den compares with 1/2 (-1 below, 0 equal, 1 above) and
// whether it is zero, on limbs.  Restoring division: Q < 2^24, one compare-and-subtract a bit.
DLIOM_FT_HD uint32_t ft_quotient_wide(uint32_t m, int e, int s, int* half, bool* exact, uint32_t bits) {
  FtWide num{m, 0u, 0u, 0u, 0u}, den{1u, 0u, 0u, 0u, 0u};
  ft_scale(num, s > 0 ? s : 0, e + s > 0 ? e + s : 0);
  ft_scale(den, s < 0 ? -s : 0, -e - s > 0 ? -e - s : 0);
  DLIOM_FT_ASSERT(num.w4 < 4u, bits);      // num < 2^130
  DLIOM_FT_ASSERT(den.w3 < 4096u && den.w4 == 0u, bits);  // den < 2^108
  [[maybe_unused]] const FtWide den0 = den;
  ft_mul_small(den, 1u << 24);
  DLIOM_FT_ASSERT(!ft_ge(num, den), bits);  // Q < 2^24
  uint32_t q = 0u;
  for (int bit = 23; bit >= 0; --bit) {
    ft_shr1(den);
    if (ft_ge(num, den)) {
      ft_sub(num, den);
      q |= 1u << bit;
    }
  }
  DLIOM_FT_ASSERT(ft_equal(den, den0) && !ft_ge(num, den), bits);
  *exact = (num.w0 | num.w1 | num.w2 | num.w3 | num.w4) == 0u;
  ft_mul_small(num, 2u);  // 2 * rem against den
  *half = ft_equal(num, den) ? 0 : ft_ge(num, den) ? 1 : -1;
  return q;
}

// The same in 64-bit words, for -13 <= s <= 13 (that is -8 <= X0 <= 18).
DLIOM_FT_HD uint32_t ft_quotient_word(uint32_t m, int e, int s, int* half, bool* exact, uint32_t bits) {
  uint64_t q, rem, den;
  if (s >= 0) {
    // v < 10^(X0 + 2) makes e + s negative for every such float: den is a power of two
    DLIOM_FT_ASSERT(e + s < 0 && -e - s <= 61, bits);
    const uint64_t num = static_cast<uint64_t>(m) * ft_pow5(s);  // < 2^55
    const int k = -e - s;
    den = uint64_t{1} << k;
    q = num >> k;
    rem = num & (den - 1u);
  } else {
    const int up = e + s > 0 ? e + s : 0, down = -e - s > 0 ? -e - s : 0;
    DLIOM_FT_ASSERT(up <= 39 && down <= 30, bits);
    const uint64_t num = static_cast<uint64_t>(m) << up;  // < 2^63
    den = static_cast<uint64_t>(ft_pow5(-s)) << down;     // < 2^61
    q = num / den;
    rem = num - q * den;
  }
  DLIOM_FT_ASSERT(q < (1u << 24), bits);
  *exact = rem == 0u;
  *half = 2u * rem == den ? 0 : 2u * rem > den ? 1 : -1;
  return static_cast<uint32_t>(q);
}

// `wide` (may be null) is set to 1 when the value took the multiword path, else to 0.
DLIOM_FT_HD FloatText float_text_of_bits(uint32_t bits, int* wide = nullptr) {
  FloatText t{0u, 0u, 0};
  if (wide != nullptr) *wide = 0;
  const uint32_t field = (bits >> 23) & 0xffu, frac = bits & 0x7fffffu;
  if (bits >> 31) ft_put(t, '-');
  if (field == 0xffu) {
    if (frac != 0u) {
      ft_put(t, 'n');
      ft_put(t, 'a');
      ft_put(t, 'n');
    } else {
      ft_put(t, 'i');
      ft_put(t, 'n');
      ft_put(t, 'f');
    }
    return t;
  }
  if (field == 0u && frac == 0u) {
    ft_put(t, '0');
    return t;
  }
  const uint32_t m = field != 0u ? frac | 0x800000u : frac;
  const int e = field != 0u ? static_cast<int>(field) - 150 : -149;
  const int l2 = e + 31 - __builtin_clz(m);  // m != 0
  // floor(l2 * 1233 / 4096) without shifting a negative number
  int x = static_cast<int>(static_cast<uint32_t>(l2 * 1233 + 256 * 4096) >> 12) - 256;
  const int s = 5 - x;
  int half;
  bool exact;
  uint32_t q;
  if (s >= -13 && s <= 13) {
    q = ft_quotient_word(m, e, s, &half, &exact, bits);
  } else {
    if (wide != nullptr) *wide = 1;
    q = ft_quotient_wide(m, e, s, &half, &exact, bits);
  }
  DLIOM_FT_ASSERT(q >= 100000u && q < 10000000u, bits);
  uint32_t d = q;
  if (q >= 1000000u) {  // the estimate was one short: one more digit to discard
    d = q / 10u;
    const uint32_t last = q - d * 10u;
    half = last > 5u ? 1 : last < 5u ? -1 : exact ? 0 : 1;
    ++x;
  }
  d += (half > 0 || (half == 0 && (d & 1u) != 0u)) ? 1u : 0u;
  if (d == 1000000u) {
    d = 100000u;
    ++x;
  }
  int digits = 6;  // without the trailing zeros
  for (uint32_t r = d; r % 10u == 0u; r /= 10u) --digits;
  const bool fixed = x >= -4 && x < 6;
  int point = 1;  // digits in front of the '.'
  int count = digits;
  if (fixed && x < 0) {
    ft_put(t, '0');
    ft_put(t, '.');
    for (int i = 1; i < -x; ++i) ft_put(t, '0');
    point = 0;
  } else if (fixed) {
    point = x + 1;
    count = digits > point ? digits : point;  // the integer part's own zeros are digits of d
  }
  for (int i = 0; i < count; ++i) {
    if (i == point && i > 0) ft_put(t, '.');
    const uint32_t digit = d / 100000u;
    d = (d - digit * 100000u) * 10u;
    ft_put(t, '0' + digit);
  }
  if (!fixed) {
    ft_put(t, 'e');
    ft_put(t, x < 0 ? '-' : '+');
    const uint32_t ax = static_cast<uint32_t>(x < 0 ? -x : x);  // <= 45
    ft_put(t, '0' + ax / 10u);
    ft_put(t, '0' + ax % 10u);
  }
  DLIOM_FT_ASSERT(t.length <= kFloatTextMax, bits);
  return t;
}

}  // namespace dliom

#endif  // DLIOM_CSRC_FLOAT_TEXT_H_
