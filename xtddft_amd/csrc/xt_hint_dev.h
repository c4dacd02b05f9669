// Device functions shared by the kernels that work on Hermite-form distributions with stated
// orders (xt_hint.hip, xt_grad.hip): the Boys table for total orders up to kHintMaxL and the
// Hermite Coulomb integrals R_tuv.  Every unit that includes this header owns a copy of the
// table (no relocatable device code), filled once per device by hint_boys_ensure().
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <mutex>
#include "xt_internal.h"
#include "xt_hermite.h"

namespace xt {

// F_n(T_i), T_i = i h on [0, 30], n <= HB_NM - 1, and the 7-term Taylor series about the
// nearest T_i: the scheme of xt_int.hip's table (remainder ~1.2e-15 relative) at more orders
constexpr int HB_NM = kHintMaxL + 7;
constexpr int HB_NT = 601;
constexpr double HB_H = 0.05;
static __device__ double g_hint_boys[HB_NT * HB_NM];

static __global__ void k_hint_boys_init() {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < HB_NT) {
    double F[HB_NM];
    boys_series(HB_NM - 1, i * HB_H, F);
    for (int n = 0; n < HB_NM; ++n) g_hint_boys[i * HB_NM + n] = F[n];
  }
}

__device__ __forceinline__ void hint_boys(int m, double T, double* F) {
  if (T < 30.0) {
    const int i = (int)(T * (1.0 / HB_H) + 0.5);
    const double md = i * HB_H - T;
    const double* f = g_hint_boys + i * HB_NM + m;
    double v = f[6];
#pragma unroll
    for (int k = 5; k >= 0; --k) v = f[k] + md * (1.0 / (k + 1)) * v;
    F[m] = v;
    const double et = exp(-T);
    for (int n = m - 1; n >= 0; --n) F[n] = (2.0 * T * F[n + 1] + et) * (1.0 / (2 * n + 1));
  } else {
    boys_series(m, T, F);   // upward from F_0: (2n + 1) / (2T) < 1 for n <= 14 < T
  }
}

// R^0_tuv(alpha, X, Y, Z), t + u + v <= L (qc/ints.py hermite_r): two level buffers, result in R
template <int MAXL>
__device__ void hint_r(int L, double alpha, double X, double Y, double Z, double* R, double* S) {
  double F[MAXL + 1];
  hint_boys(L, alpha * (X * X + Y * Y + Z * Z), F);
  const double m2a = -2.0 * alpha;
  double pw = 1.0;
  for (int n = 0; n < L; ++n) pw *= m2a;
  double* prev = R;
  double* cur = S;
  if (L % 2) { prev = S; cur = R; }
  prev[0] = pw * F[L];
  for (int n = L - 1; n >= 0; --n) {
    pw /= m2a;
    cur[0] = pw * F[n];
    for (int tot = 1; tot <= L - n; ++tot)
      for (int t = tot; t >= 0; --t)
        for (int u = tot - t; u >= 0; --u) {
          const int v = tot - t - u;
          double val;
          if (t > 0) {
            val = X * prev[tuv_pos(t - 1, u, v)];
            if (t > 1) val += (t - 1) * prev[tuv_pos(t - 2, u, v)];
          } else if (u > 0) {
            val = Y * prev[tuv_pos(0, u - 1, v)];
            if (u > 1) val += (u - 1) * prev[tuv_pos(0, u - 2, v)];
          } else {
            val = Z * prev[tuv_pos(0, 0, v - 1)];
            if (v > 1) val += (v - 1) * prev[tuv_pos(0, 0, v - 2)];
          }
          cur[tuv_pos(t, u, v)] = val;
        }
    double* tmp = prev; prev = cur; cur = tmp;
  }
}

// this unit's Boys table, once per device (stream-ordered before the caller's launch)
static int hint_boys_ensure(hipStream_t st) {
  static std::mutex mu;
  static unsigned long long done = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(mu);
  if (dev >= 64 || !(done >> dev & 1ull)) {
    hipLaunchKernelGGL(k_hint_boys_init, dim3((HB_NT + 63) / 64), dim3(64), 0, st);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return XT_ERR_HIP;
    if (dev < 64) done |= 1ull << dev;
  }
  return 0;
}

}  // namespace xt
