// The host's solver for the small symmetric systems of the gravity estimates (imu_window.cc: GravityEstimator, 3 and 2
// columns; imu_lidar_init.cc: Initializer, 3 N + 3 and 3 N + 2 columns), stated once.  It stands for Eigen's A.ldlt().solve(b)
// and is PARITY UNPINNED AGAINST EIGEN: Gaussian elimination with partial pivoting by rows (the largest |entry| of the
// column, ties the first), the row operations in ascending row and column order, then back substitution with the sums
// taken left to right.  false: a column without a non-zero pivot.
#ifndef DLIOM_CSRC_SYM_SOLVE_H_
#define DLIOM_CSRC_SYM_SOLVE_H_

#include <cmath>
#include <utility>
#include <vector>

namespace dliom {

inline bool solve_sym(const double* A, const double* b, int n, double* x) {
  const int w = n + 1;
  double small[12];  // GravityEstimator's 2- and 3-column systems stay off the heap
  std::vector<double> large;
  if (n > 3) large.resize(static_cast<size_t>(n) * w);
  double* const M = n > 3 ? large.data() : small;
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) M[i * w + j] = A[i * n + j];
    M[i * w + n] = b[i];
  }
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(M[r * w + c]) > std::fabs(M[piv * w + c])) piv = r;
    if (!(std::fabs(M[piv * w + c]) > 0.0)) return false;
    for (int j = 0; j <= n; ++j) std::swap(M[c * w + j], M[piv * w + j]);
    for (int r = c + 1; r < n; ++r) {
      const double f = M[r * w + c] / M[c * w + c];
      for (int j = c; j <= n; ++j) M[r * w + j] -= f * M[c * w + j];
    }
  }
  for (int i = n - 1; i >= 0; --i) {
    double v = M[i * w + n];
    for (int j = i + 1; j < n; ++j) v -= M[i * w + j] * x[j];
    x[i] = v / M[i * w + i];
  }
  return true;
}

}  // namespace dliom

#endif  // DLIOM_CSRC_SYM_SOLVE_H_
