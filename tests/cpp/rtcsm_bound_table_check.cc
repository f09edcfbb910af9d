// The per-match table of the sequential sum's error bound (d-liom_amd/csrc/rtcsm_bounds.h) against the loop it replaces
// in rtcsm_bounds_kernel: for n = 1, 64, 170, 65 536, 262 144 and 2^19 points and U at both ends and in the middle of
// every binade from 2^-4 to 2^20, on the doubles' bits; and the corners the kernel can meet outside that range (a U
// below 2^-4, zero, negative, huge, infinite, NaN).
// Stand-alone: g++ -std=c++17 -O3 -ffp-contract=off (the library's host flags), and once more with
// -fsanitize=address,undefined.  Prints "ok cases <comparisons>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../d-liom_amd/csrc/rtcsm_bounds.h"

using namespace dliom;

namespace {
uint64_t bits_of(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return b;
}
long long g_cases = 0;
bool same(int n, const SeqSumBoundTable& t, double U) {
  ++g_cases;
  const double want = seq_sum_error_bound(n, U), got = t.err[seq_sum_bound_index(U)];
  if (bits_of(want) == bits_of(got)) return true;
  std::printf("FAIL n %d U %a: loop %a table %a (index %d)\n", n, U, want, got, seq_sum_bound_index(U));
  return false;
}
}  // namespace

int main() {
  const int ns[] = {1, 64, 170, 65536, 262144, 1 << 19};
  bool ok = true;
  for (int n : ns) {
    SeqSumBoundTable t;
    fill_seq_sum_bound_table(n, &t);
    for (int K = -4; K <= 20; ++K) {
      const double lo = std::ldexp(1.0, K), next = std::ldexp(1.0, K + 1);
      ok = same(n, t, lo) && ok;                                  // the binade's first double
      ok = same(n, t, std::nextafter(lo, next)) && ok;            // ... and the one behind it
      ok = same(n, t, 1.5 * lo) && ok;                            // the middle
      ok = same(n, t, std::nextafter(next, 0.0)) && ok;           // the binade's last double
    }
    const double corners[] = {0.0, -1.0, std::numeric_limits<double>::denorm_min(), std::ldexp(1.0, -5), std::nextafter(0.0625, 0.0),
                              std::ldexp(1.0, 21), std::ldexp(1.0, 62), std::ldexp(1.0, 63), std::ldexp(1.5, 63), std::ldexp(1.0, 64),
                              std::ldexp(1.0, 300), std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()};
    for (double U : corners) ok = same(n, t, U) && ok;
  }
  if (!ok) return 1;
  std::printf("ok cases %lld\n", g_cases);
  return 0;
}
