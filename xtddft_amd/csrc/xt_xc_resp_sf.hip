// The grid work of the multicollinear spin-flip TDA gradient on a UKS reference that is not a GEMM
// (xtddft_amd/qc/device.py DeviceEngine.fxc_sf_response / rows_potential).
//
// xt_xc_resp_sf: one spin-flip channel.  With c = phi X_S from the caller,
//
//   rho1(0, g) = sum_mu phi_mu(g) c(g, mu)            rho1(k, g) = 2 sum_mu d_k phi_mu(g) c(g, mu)
//   wv(k, g)   = 2 w_g sum_k' fxc_sf(k, k', g) rho1(k', g)                              (nothing halved)
//   b(g, mu)   = 1/2 wv(0, g) phi_mu(g) + sum_k wv(k, g) d_k phi_mu(g)                  (GGA)
//   b(g, mu)   = wv(0, g) phi_mu(g)                                                     (LDA)
//
// xt_xc_rows: b_ch(g, mu) of given weights wv[(4 ch + k) ldo + g] for nch = 1..4 channels, the AO rows
// read once for all of them: the third pass of xt_xc_resp on its own, with its arithmetic (`xs_rows`
// below is that pass for NCH channels), so that on the weights xt_xc_resp wrote it gives that call's b
// bit for bit.
//
// As in xt_xc_resp.hip a block of four waves owns 64 consecutive grid points:
//   1. wave q reduces rows 16 q .. 16 q + 15, lanes striding over mu two AOs at a time (16-byte loads
//      where the operands allow, `VEC`), an xor butterfly folds the dot products and lane 0 puts rho1
//      into LDS;
//   2. after a barrier thread (q, p) is point p: wave q contracts row q of the point's 4 x 4 fxc_sf
//      block (LDA: wave 0, the one entry), writes rho1 and wv and leaves wv in LDS;
//   3. after a second barrier the waves stream their rows again and write b.
// No atomics, and a summation order that does not depend on the alignment path: equal inputs give
// equal bits.  Weights of zero give b = 0 for finite AO values; fxc_sf = 0 at a point gives wv = 0 there
// as long as rho1 is finite.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "xt_host.h"
#include "xt_internal.h"

namespace xt {

constexpr int kXsTile = 64;      // grid points per block
constexpr int kXsBlock = 256;    // four waves
constexpr int kXsRows = kXsTile / (kXsBlock / 64);

// two consecutive doubles at p; `two` false: the row ends after the first
template <bool VEC>
__device__ __forceinline__ double2 xs_load2(const double* __restrict__ p, bool two) {
  if (VEC) {
    if (two) return *reinterpret_cast<const double2*>(p);
    return make_double2(p[0], 0.0);
  }
  return make_double2(p[0], two ? p[1] : 0.0);
}

template <bool VEC>
__device__ __forceinline__ void xs_store2(double* __restrict__ p, double2 v, bool two) {
  if (VEC && two) {
    *reinterpret_cast<double2*>(p) = v;
  } else {
    p[0] = v.x;
    if (two) p[1] = v.y;
  }
}

__device__ __forceinline__ double xs_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// b_ch(g, mu) for the rows of wave q from the weights in LDS, s_wv[4 ch + k][point of the tile]; the
// AO rows are loaded once and serve every channel.  b[(ch ngrid + g) ldb + mu].
template <bool GGA, bool VEC, int NCH>
__device__ __forceinline__ void xs_rows(long ngrid, int nao, const double* __restrict__ ao, long ao_plane,
                                        long ldao, const double (*s_wv)[kXsTile], double* __restrict__ b,
                                        long ldb, long g0, int q, int lane) {
  for (int r = q * kXsRows; r < (q + 1) * kXsRows; ++r) {
    const long g = g0 + r;
    if (g >= ngrid) break;
    const double* a0 = ao + g * ldao;
    double h[NCH][4];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      h[ch][0] = GGA ? 0.5 * s_wv[4 * ch][r] : s_wv[4 * ch][r];
#pragma unroll
      for (int k = 1; k < 4; ++k) h[ch][k] = GGA ? s_wv[4 * ch + k][r] : 0.0;
    }
    for (int mu = 2 * lane; mu < nao; mu += 128) {
      const bool two = mu + 1 < nao;
      const double2 f0 = xs_load2<VEC>(a0 + mu, two);
      double2 f1 = make_double2(0.0, 0.0), f2 = f1, f3 = f1;
      if (GGA) {
        f1 = xs_load2<VEC>(a0 + ao_plane + mu, two);
        f2 = xs_load2<VEC>(a0 + 2 * ao_plane + mu, two);
        f3 = xs_load2<VEC>(a0 + 3 * ao_plane + mu, two);
      }
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        double2 o = make_double2(h[ch][0] * f0.x, h[ch][0] * f0.y);
        if (GGA) {
          o.x = fma(h[ch][3], f3.x, fma(h[ch][2], f2.x, fma(h[ch][1], f1.x, o.x)));
          o.y = fma(h[ch][3], f3.y, fma(h[ch][2], f2.y, fma(h[ch][1], f1.y, o.y)));
        }
        xs_store2<VEC>(b + ((long)ch * ngrid + g) * ldb + mu, o, two);
      }
    }
  }
}

template <bool GGA, bool VEC>
__global__ void __launch_bounds__(kXsBlock)
k_xc_resp_sf(long ngrid, int nao, const double* __restrict__ ao, long ao_plane, long ldao,
             const double* __restrict__ c, long ldc, const double* __restrict__ fxc, long ldg,
             const double* __restrict__ w, double* __restrict__ rho1, double* __restrict__ wv, long ldo,
             double* __restrict__ b, long ldb) {
  constexpr int NC = GGA ? 4 : 1;
  __shared__ double s_rho[4][kXsTile];
  __shared__ double s_wv[4][kXsTile];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const long g0 = (long)blockIdx.x * kXsTile;

  // ---- 1. rho1 of the wave's rows
  for (int r = q * kXsRows; r < (q + 1) * kXsRows; ++r) {
    const long g = g0 + r;
    if (g >= ngrid) break;
    const double* a0 = ao + g * ldao;
    const double* cg = c + g * ldc;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
    for (int mu = 2 * lane; mu < nao; mu += 128) {
      const bool two = mu + 1 < nao;
      const double2 v = xs_load2<VEC>(cg + mu, two);
      const double2 f0 = xs_load2<VEC>(a0 + mu, two);
      p0 = fma(f0.y, v.y, fma(f0.x, v.x, p0));
      if (GGA) {
        const double2 f1 = xs_load2<VEC>(a0 + ao_plane + mu, two);
        const double2 f2 = xs_load2<VEC>(a0 + 2 * ao_plane + mu, two);
        const double2 f3 = xs_load2<VEC>(a0 + 3 * ao_plane + mu, two);
        p1 = fma(f1.y, v.y, fma(f1.x, v.x, p1));
        p2 = fma(f2.y, v.y, fma(f2.x, v.x, p2));
        p3 = fma(f3.y, v.y, fma(f3.x, v.x, p3));
      }
    }
    p0 = xs_wave_sum(p0);
    if (GGA) {
      p1 = 2.0 * xs_wave_sum(p1); p2 = 2.0 * xs_wave_sum(p2); p3 = 2.0 * xs_wave_sum(p3);
    }
    if (lane == 0) {
      s_rho[0][r] = p0;
      if (GGA) {
        s_rho[1][r] = p1; s_rho[2][r] = p2; s_rho[3][r] = p3;
      }
    }
  }
  __syncthreads();

  // ---- 2. lane = point: wave q contracts row q of the fxc_sf block (LDA: wave 0)
  {
    const long g = g0 + lane;
    if (g < ngrid && q < NC) {
      const double* f = fxc + (long)q * NC * ldg + g;
      double acc = 0.0;
#pragma unroll
      for (int k2 = 0; k2 < NC; ++k2) acc = fma(f[(long)k2 * ldg], s_rho[k2][lane], acc);
      const double v = 2.0 * (w[g] * acc);
      s_wv[q][lane] = v;
      if (wv) wv[(long)q * ldo + g] = v;
      if (rho1) rho1[(long)q * ldo + g] = s_rho[q][lane];
    }
  }
  if (!b) return;
  __syncthreads();

  // ---- 3. b of the wave's rows
  xs_rows<GGA, VEC, 1>(ngrid, nao, ao, ao_plane, ldao, s_wv, b, ldb, g0, q, lane);
}

template <bool GGA, bool VEC, int NCH>
__global__ void __launch_bounds__(kXsBlock)
k_xc_rows(long ngrid, int nao, const double* __restrict__ ao, long ao_plane, long ldao,
          const double* __restrict__ wv, long ldo, double* __restrict__ b, long ldb) {
  constexpr int NC = GGA ? 4 : 1;
  __shared__ double s_wv[4 * NCH][kXsTile];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const long g0 = (long)blockIdx.x * kXsTile;
  // the weights of the tile: wave q brings planes q, q + 4, ... of the NCH * NC that are read
  for (int i = q; i < NCH * NC; i += kXsBlock / 64) {
    const int slot = GGA ? i : 4 * i;            // 4 ch + k
    const long g = g0 + lane;
    s_wv[slot][lane] = g < ngrid ? wv[(long)slot * ldo + g] : 0.0;
  }
  __syncthreads();
  xs_rows<GGA, VEC, NCH>(ngrid, nao, ao, ao_plane, ldao, s_wv, b, ldb, g0, q, lane);
}

static bool xs_even16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool GGA, bool VEC>
static void xs_launch_rows(int nch, unsigned nblock, hipStream_t st, long ngrid, int nao, const double* ao,
                           long ao_plane, long ldao, const double* wv, long ldo, double* b, long ldb) {
#define XT_XS_ROWS(N)                                                                                     \
  hipLaunchKernelGGL((k_xc_rows<GGA, VEC, N>), dim3(nblock), dim3(kXsBlock), 0, st, ngrid, nao, ao, ao_plane, \
                     ldao, wv, ldo, b, ldb)
  switch (nch) {
    case 1: XT_XS_ROWS(1); break;
    case 2: XT_XS_ROWS(2); break;
    case 3: XT_XS_ROWS(3); break;
    default: XT_XS_ROWS(4); break;
  }
#undef XT_XS_ROWS
}

}  // namespace xt

using namespace xt;

extern "C" int xt_xc_resp_sf(long ngrid, int nao, int xctype, const double* ao, long ao_plane, long ldao,
                             const double* c, long ldc, const double* fxc_sf, long ldg, const double* w,
                             double* rho1, double* wv, long ldo, double* b, long ldb, void* stream) {
  if (ngrid < 0 || nao < 0 || ao_plane < 0 || ldao < 0 || ldc < 0 || ldg < 0 || ldo < 0 || ldb < 0)
    return fail(XT_ERR_ARG, "xt_xc_resp_sf: negative size");
  if (xctype != XT_XC_LDA && xctype != XT_XC_GGA)
    return fail(XT_ERR_ARG, "xt_xc_resp_sf: xctype must be XT_XC_LDA or XT_XC_GGA");
  const bool gga = xctype == XT_XC_GGA;
  if (ldao < nao) return fail(XT_ERR_ARG, "xt_xc_resp_sf: ldao < nao");
  if (ldc < nao) return fail(XT_ERR_ARG, "xt_xc_resp_sf: ldc < nao");
  if (b && ldb < nao) return fail(XT_ERR_ARG, "xt_xc_resp_sf: ldb < nao");
  if (ldg < ngrid) return fail(XT_ERR_ARG, "xt_xc_resp_sf: ldg < ngrid");
  if ((rho1 || wv) && ldo < ngrid) return fail(XT_ERR_ARG, "xt_xc_resp_sf: ldo < ngrid");
  if (gga && ngrid > 0 && nao > 0 && ao_plane < (ngrid - 1) * ldao + nao)
    return fail(XT_ERR_ARG, "xt_xc_resp_sf: ao_plane shorter than the rows of one plane");
  const long nblock = (ngrid + kXsTile - 1) / kXsTile;
  if (nblock > INT_MAX) return fail(XT_ERR_ARG, "xt_xc_resp_sf: more than 2^31 blocks, split the grid");
  if (ngrid == 0 || nao == 0 || (!rho1 && !wv && !b)) return 0;
  if (!ao || !c || !fxc_sf || !w) return fail(XT_ERR_ARG, "xt_xc_resp_sf: null ao, c, fxc_sf or w");
  // 16-byte accesses: every row that is read or written two AOs at a time starts on a 16-byte boundary
  const bool vec = xs_even16(ao) && xs_even16(c) && (!b || xs_even16(b)) && ldao % 2 == 0 && ldc % 2 == 0 &&
                   (!b || ldb % 2 == 0) && (!gga || ao_plane % 2 == 0);
  hipStream_t st = (hipStream_t)stream;
#define XT_XS_RUN(G, V)                                                                                         \
  hipLaunchKernelGGL((k_xc_resp_sf<G, V>), dim3((unsigned)nblock), dim3(kXsBlock), 0, st, ngrid, nao, ao, ao_plane, \
                     ldao, c, ldc, fxc_sf, ldg, w, rho1, wv, ldo, b, ldb)
  if (gga) {
    if (vec) XT_XS_RUN(true, true); else XT_XS_RUN(true, false);
  } else {
    if (vec) XT_XS_RUN(false, true); else XT_XS_RUN(false, false);
  }
#undef XT_XS_RUN
  return hipGetLastError() == hipSuccess ? 0 : fail(XT_ERR_HIP, "xt_xc_resp_sf: launch failed");
}

extern "C" int xt_xc_rows(long ngrid, int nao, int xctype, int nch, const double* ao, long ao_plane, long ldao,
                          const double* wv, long ldo, double* b, long ldb, void* stream) {
  if (ngrid < 0 || nao < 0 || ao_plane < 0 || ldao < 0 || ldo < 0 || ldb < 0)
    return fail(XT_ERR_ARG, "xt_xc_rows: negative size");
  if (xctype != XT_XC_LDA && xctype != XT_XC_GGA)
    return fail(XT_ERR_ARG, "xt_xc_rows: xctype must be XT_XC_LDA or XT_XC_GGA");
  if (nch < 1 || nch > 4) return fail(XT_ERR_ARG, "xt_xc_rows: nch must be 1..4");
  const bool gga = xctype == XT_XC_GGA;
  if (ldao < nao) return fail(XT_ERR_ARG, "xt_xc_rows: ldao < nao");
  if (b && ldb < nao) return fail(XT_ERR_ARG, "xt_xc_rows: ldb < nao");
  if (ldo < ngrid) return fail(XT_ERR_ARG, "xt_xc_rows: ldo < ngrid");
  if (gga && ngrid > 0 && nao > 0 && ao_plane < (ngrid - 1) * ldao + nao)
    return fail(XT_ERR_ARG, "xt_xc_rows: ao_plane shorter than the rows of one plane");
  const long nblock = (ngrid + kXsTile - 1) / kXsTile;
  if (nblock > INT_MAX) return fail(XT_ERR_ARG, "xt_xc_rows: more than 2^31 blocks, split the grid");
  if (ngrid == 0 || nao == 0 || !b) return 0;
  if (!ao || !wv) return fail(XT_ERR_ARG, "xt_xc_rows: null ao or wv");
  const bool vec = xs_even16(ao) && xs_even16(b) && ldao % 2 == 0 && ldb % 2 == 0 && (!gga || ao_plane % 2 == 0) &&
                   (nch == 1 || (ngrid * ldb) % 2 == 0);
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)nblock;
  if (gga) {
    if (vec) xs_launch_rows<true, true>(nch, nb, st, ngrid, nao, ao, ao_plane, ldao, wv, ldo, b, ldb);
    else xs_launch_rows<true, false>(nch, nb, st, ngrid, nao, ao, ao_plane, ldao, wv, ldo, b, ldb);
  } else {
    if (vec) xs_launch_rows<false, true>(nch, nb, st, ngrid, nao, ao, ao_plane, ldao, wv, ldo, b, ldb);
    else xs_launch_rows<false, false>(nch, nb, st, ngrid, nao, ao, ao_plane, ldao, wv, ldo, b, ldb);
  }
  return hipGetLastError() == hipSuccess ? 0 : fail(XT_ERR_HIP, "xt_xc_rows: launch failed");
}
