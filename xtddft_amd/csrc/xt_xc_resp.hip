// The exchange-correlation linear response of a UKS reference in the AO route, everything that is
// not a GEMM (xtddft_amd/qc/device.py DeviceEngine.fxc_response; the XC part of the UKS
// gen_response(hermi=1) the Z-vector equations of the spin-flip TDA gradient apply, and the f^xc[T]
// of their right-hand side): for symmetric trial densities dm_s, with c_s = phi dm_s from the caller,
//
//   rho1_s(0, g) = sum_mu phi_mu(g) c_s(g, mu)        rho1_s(k, g) = 2 sum_mu d_k phi_mu(g) c_s(g, mu)
//   wv_s(k, g)   = w_g sum_{s' k'} fxc(s, k, s', k', g) rho1_s'(k', g)                  (nothing halved)
//   b_s(g, mu)   = 1/2 wv_s(0, g) phi_mu(g) + sum_k wv_s(k, g) d_k phi_mu(g)            (GGA)
//   b_s(g, mu)   = wv_s(0, g) phi_mu(g)                                                 (LDA)
//
// so that V^resp_s = phi^T b_s (+ its transpose for GGA) is one GEMM per spin for the caller.
//
// A block of four waves owns 64 consecutive grid points.
//   1. Wave q reduces rows 16 q .. 16 q + 15: its lanes stride over mu two AOs at a time (16-byte
//      loads where the operands allow, see `VEC`), the 2 ncomp dot products of a row are folded by
//      an xor butterfly, which leaves the same bits in every lane, and lane 0 puts rho1 into LDS.
//   2. After a barrier thread (q, p) is point p: wave q contracts rows 2 q and 2 q + 1 of the
//      point's 8 x 8 fxc column block (LDA: waves 0 and 1, one row of the 2 x 2 each), reading each
//      entry once and coalesced along g, writes rho1 and wv and leaves wv in LDS.
//   3. After a second barrier the waves stream their rows again (the AO rows come from L2) and
//      write b for both spins.
// No atomics and a fixed summation order that does not depend on the alignment path: equal inputs
// give equal bits.  A point whose fxc entries are all zero gets wv = 0 and b = 0 as long as rho1 is
// finite there (0 x Inf is NaN: a c that holds Inf or NaN at a screened point is not cleaned up).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "xt_host.h"
#include "xt_internal.h"

namespace xt {

constexpr int kXrTile = 64;      // grid points per block
constexpr int kXrBlock = 256;    // four waves
constexpr int kXrRows = kXrTile / (kXrBlock / 64);

// two consecutive doubles at p; `two` false: the row ends after the first
template <bool VEC>
__device__ __forceinline__ double2 xr_load2(const double* __restrict__ p, bool two) {
  if (VEC) {
    if (two) return *reinterpret_cast<const double2*>(p);
    return make_double2(p[0], 0.0);
  }
  return make_double2(p[0], two ? p[1] : 0.0);
}

template <bool VEC>
__device__ __forceinline__ void xr_store2(double* __restrict__ p, double2 v, bool two) {
  if (VEC && two) {
    *reinterpret_cast<double2*>(p) = v;
  } else {
    p[0] = v.x;
    if (two) p[1] = v.y;
  }
}

__device__ __forceinline__ double xr_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <bool GGA, bool VEC>
__global__ void __launch_bounds__(kXrBlock)
k_xc_resp(long ngrid, int nao, const double* __restrict__ ao, long ao_plane, long ldao,
          const double* __restrict__ c, long ldc, const double* __restrict__ fxc, long ldg,
          const double* __restrict__ w, double* __restrict__ rho1, double* __restrict__ wv, long ldo,
          double* __restrict__ b, long ldb) {
  constexpr int NC = GGA ? 4 : 1;
  __shared__ double s_rho[8][kXrTile];
  __shared__ double s_wv[8][kXrTile];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const long g0 = (long)blockIdx.x * kXrTile;

  // ---- 1. rho1 of the wave's rows
  for (int r = q * kXrRows; r < (q + 1) * kXrRows; ++r) {
    const long g = g0 + r;
    if (g >= ngrid) break;
    const double* a0 = ao + g * ldao;
    const double* ca = c + g * ldc;
    const double* cb = c + (ngrid + g) * ldc;
    double pa0 = 0.0, pa1 = 0.0, pa2 = 0.0, pa3 = 0.0, pb0 = 0.0, pb1 = 0.0, pb2 = 0.0, pb3 = 0.0;
    for (int mu = 2 * lane; mu < nao; mu += 128) {
      const bool two = mu + 1 < nao;
      const double2 va = xr_load2<VEC>(ca + mu, two), vb = xr_load2<VEC>(cb + mu, two);
      const double2 f0 = xr_load2<VEC>(a0 + mu, two);
      pa0 = fma(f0.y, va.y, fma(f0.x, va.x, pa0));
      pb0 = fma(f0.y, vb.y, fma(f0.x, vb.x, pb0));
      if (GGA) {
        const double2 f1 = xr_load2<VEC>(a0 + ao_plane + mu, two);
        const double2 f2 = xr_load2<VEC>(a0 + 2 * ao_plane + mu, two);
        const double2 f3 = xr_load2<VEC>(a0 + 3 * ao_plane + mu, two);
        pa1 = fma(f1.y, va.y, fma(f1.x, va.x, pa1));
        pb1 = fma(f1.y, vb.y, fma(f1.x, vb.x, pb1));
        pa2 = fma(f2.y, va.y, fma(f2.x, va.x, pa2));
        pb2 = fma(f2.y, vb.y, fma(f2.x, vb.x, pb2));
        pa3 = fma(f3.y, va.y, fma(f3.x, va.x, pa3));
        pb3 = fma(f3.y, vb.y, fma(f3.x, vb.x, pb3));
      }
    }
    pa0 = xr_wave_sum(pa0);
    pb0 = xr_wave_sum(pb0);
    if (GGA) {
      pa1 = 2.0 * xr_wave_sum(pa1); pa2 = 2.0 * xr_wave_sum(pa2); pa3 = 2.0 * xr_wave_sum(pa3);
      pb1 = 2.0 * xr_wave_sum(pb1); pb2 = 2.0 * xr_wave_sum(pb2); pb3 = 2.0 * xr_wave_sum(pb3);
    }
    if (lane == 0) {
      s_rho[0][r] = pa0;
      s_rho[4][r] = pb0;
      if (GGA) {
        s_rho[1][r] = pa1; s_rho[2][r] = pa2; s_rho[3][r] = pa3;
        s_rho[5][r] = pb1; s_rho[6][r] = pb2; s_rho[7][r] = pb3;
      }
    }
  }
  __syncthreads();

  // ---- 2. lane = point: rows (s, k) of the fxc contraction, two per wave (LDA: one, waves 0 and 1)
  {
    const long g = g0 + lane;
    constexpr int PER = GGA ? 2 : 1;
    if (g < ngrid && (GGA || q < 2)) {
      const double wg = w[g];
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int o = GGA ? 2 * q + i : q;            // row s * NC + k of the (2 NC) x (2 NC) block
        const int slot = GGA ? o : 4 * o;             // s * 4 + k
        const double* f = fxc + (long)o * (2 * NC) * ldg + g;
        double acc = 0.0;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int k2 = 0; k2 < NC; ++k2)
            acc = fma(f[(long)(s2 * NC + k2) * ldg], s_rho[4 * s2 + k2][lane], acc);
        const double v = wg * acc;
        s_wv[slot][lane] = v;
        if (wv) wv[(long)slot * ldo + g] = v;
        if (rho1) rho1[(long)slot * ldo + g] = s_rho[slot][lane];
      }
    }
  }
  if (!b) return;
  __syncthreads();

  // ---- 3. b of the wave's rows, both spins
  for (int r = q * kXrRows; r < (q + 1) * kXrRows; ++r) {
    const long g = g0 + r;
    if (g >= ngrid) break;
    const double* a0 = ao + g * ldao;
    double* ba = b + g * ldb;
    double* bb = b + (ngrid + g) * ldb;
    const double ha0 = GGA ? 0.5 * s_wv[0][r] : s_wv[0][r];
    const double hb0 = GGA ? 0.5 * s_wv[4][r] : s_wv[4][r];
    double ha1 = 0.0, ha2 = 0.0, ha3 = 0.0, hb1 = 0.0, hb2 = 0.0, hb3 = 0.0;
    if (GGA) {
      ha1 = s_wv[1][r]; ha2 = s_wv[2][r]; ha3 = s_wv[3][r];
      hb1 = s_wv[5][r]; hb2 = s_wv[6][r]; hb3 = s_wv[7][r];
    }
    for (int mu = 2 * lane; mu < nao; mu += 128) {
      const bool two = mu + 1 < nao;
      const double2 f0 = xr_load2<VEC>(a0 + mu, two);
      double2 oa = make_double2(ha0 * f0.x, ha0 * f0.y);
      double2 ob = make_double2(hb0 * f0.x, hb0 * f0.y);
      if (GGA) {
        const double2 f1 = xr_load2<VEC>(a0 + ao_plane + mu, two);
        const double2 f2 = xr_load2<VEC>(a0 + 2 * ao_plane + mu, two);
        const double2 f3 = xr_load2<VEC>(a0 + 3 * ao_plane + mu, two);
        oa.x = fma(ha3, f3.x, fma(ha2, f2.x, fma(ha1, f1.x, oa.x)));
        oa.y = fma(ha3, f3.y, fma(ha2, f2.y, fma(ha1, f1.y, oa.y)));
        ob.x = fma(hb3, f3.x, fma(hb2, f2.x, fma(hb1, f1.x, ob.x)));
        ob.y = fma(hb3, f3.y, fma(hb2, f2.y, fma(hb1, f1.y, ob.y)));
      }
      xr_store2<VEC>(ba + mu, oa, two);
      xr_store2<VEC>(bb + mu, ob, two);
    }
  }
}

static bool xr_even16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace xt

using namespace xt;

extern "C" int xt_xc_resp(long ngrid, int nao, int xctype, const double* ao, long ao_plane, long ldao,
                          const double* c, long ldc, const double* fxc, long ldg, const double* w,
                          double* rho1, double* wv, long ldo, double* b, long ldb, void* stream) {
  if (ngrid < 0 || nao < 0 || ao_plane < 0 || ldao < 0 || ldc < 0 || ldg < 0 || ldo < 0 || ldb < 0)
    return fail(XT_ERR_ARG, "xt_xc_resp: negative size");
  if (xctype != XT_XC_LDA && xctype != XT_XC_GGA)
    return fail(XT_ERR_ARG, "xt_xc_resp: xctype must be XT_XC_LDA or XT_XC_GGA");
  const bool gga = xctype == XT_XC_GGA;
  if (ldao < nao) return fail(XT_ERR_ARG, "xt_xc_resp: ldao < nao");
  if (ldc < nao) return fail(XT_ERR_ARG, "xt_xc_resp: ldc < nao");
  if (b && ldb < nao) return fail(XT_ERR_ARG, "xt_xc_resp: ldb < nao");
  if (ldg < ngrid) return fail(XT_ERR_ARG, "xt_xc_resp: ldg < ngrid");
  if ((rho1 || wv) && ldo < ngrid) return fail(XT_ERR_ARG, "xt_xc_resp: ldo < ngrid");
  if (gga && ngrid > 0 && nao > 0 && ao_plane < (ngrid - 1) * ldao + nao)
    return fail(XT_ERR_ARG, "xt_xc_resp: ao_plane shorter than the rows of one plane");
  const long nblock = (ngrid + kXrTile - 1) / kXrTile;
  if (nblock > INT_MAX) return fail(XT_ERR_ARG, "xt_xc_resp: more than 2^31 blocks, split the grid");
  if (ngrid == 0 || nao == 0 || (!rho1 && !wv && !b)) return 0;
  if (!ao || !c || !fxc || !w) return fail(XT_ERR_ARG, "xt_xc_resp: null ao, c, fxc or w");
  // 16-byte accesses: every row of every operand that is read or written two AOs at a time starts
  // on a 16-byte boundary
  const bool vec = xr_even16(ao) && xr_even16(c) && (!b || xr_even16(b)) && ldao % 2 == 0 && ldc % 2 == 0 &&
                   (!b || ldb % 2 == 0) && (!gga || ao_plane % 2 == 0) && ((ngrid * ldc) % 2 == 0) &&
                   (!b || (ngrid * ldb) % 2 == 0);
  hipStream_t st = (hipStream_t)stream;
#define XT_XR_RUN(G, V)                                                                                      \
  hipLaunchKernelGGL((k_xc_resp<G, V>), dim3((unsigned)nblock), dim3(kXrBlock), 0, st, ngrid, nao, ao, ao_plane, \
                     ldao, c, ldc, fxc, ldg, w, rho1, wv, ldo, b, ldb)
  if (gga) {
    if (vec) XT_XR_RUN(true, true); else XT_XR_RUN(true, false);
  } else {
    if (vec) XT_XR_RUN(false, true); else XT_XR_RUN(false, false);
  }
#undef XT_XR_RUN
  return hipGetLastError() == hipSuccess ? 0 : fail(XT_ERR_HIP, "xt_xc_resp: launch failed");
}
