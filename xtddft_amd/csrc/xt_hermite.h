// Device helpers shared by the integral kernels (xt_int.hip, xt_hint.hip): the Hermite index
// order of qc/ints.py and the Boys function by series / recursion.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace xt {

__host__ __device__ constexpr int ntuv(int L) { return (L + 1) * (L + 2) * (L + 3) / 6; }
__host__ __device__ constexpr int ncart(int l) { return (l + 1) * (l + 2) / 2; }
// position of (t, u, v) in the order of qc/ints.py hermite_index: by n = t + u + v,
// then t descending, then u descending
__host__ __device__ constexpr int tuv_pos(int t, int u, int v) {
  const int n = t + u + v, d = n - t;
  return n * (n + 1) * (n + 2) / 6 + d * (d + 1) / 2 + (d - u);
}

// F_n(T), n = 0..m: the series for F_m and downward recursion below T = 30 (all
// terms positive, no cancellation), F_0 = sqrt(pi/T) erf(sqrt T) / 2 and upward
// recursion above (the amplification (2n+1)/(2T) < 1 for n <= 13 < T: stable).
// The series runs only to fill the table below (its ~T + 30 divisions per call made
// the Boys function the bulk of an s-shell quartet's cost).
__device__ void boys_series(int m, double T, double* F) {
  if (T < 30.0) {
    double term = 1.0 / (2 * m + 1), sum = term;
    for (int k = 1; k < 400; ++k) {
      term *= 2.0 * T / (2 * m + 2 * k + 1);
      sum += term;
      if (term < 1e-17 * sum) break;
    }
    const double et = exp(-T);
    F[m] = et * sum;
    for (int n = m - 1; n >= 0; --n) F[n] = (2.0 * T * F[n + 1] + et) / (2 * n + 1);
  } else {
    const double et = exp(-T);
    F[0] = 0.5 * sqrt(M_PI / T) * erf(sqrt(T));
    for (int n = 0; n < m; ++n) F[n + 1] = ((2 * n + 1) * F[n] - et) / (2.0 * T);
  }
}

}  // namespace xt
