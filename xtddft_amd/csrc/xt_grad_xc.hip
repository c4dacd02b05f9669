// The exchange-correlation force on the atoms at fixed spin density matrices -- the nuclear
// derivative of the XC potential matrix contracted with the ground-state density (PySCF
// grad.uks.get_vxc; the vxc1[:, 1:] of the reference's grad_hb/tduks_sfu.py:168-177), without
// grid-weight derivatives (xtddft_amd/qc/grad.py grad_xc_device):
//
//   out[3A + x] += sum_s sum_g sum_{mu on A} d_x phi_mu(g) e_s(g, mu)
//                                          + (sum_k h_s(k, g) d_x d_k phi_mu(g)) c_s(g, mu)
//
//   h[(4 s + k) ldg + g], k = 1..3   w_g d eps / d(d_k rho_s) ("eff" layout, nothing halved);
//                                    plane 0 is part of e and is never read
//   e[(s nao + mu) ldg + g]          e_s = b_s D_s,  b_s = h_s(0) phi + sum_k h_s(k) d_k phi
//   c[(s nao + mu) ldg + g]          c_s = phi D_s
//
// e and c are AO-major: the lanes of a wave are 64 consecutive grid points of ONE shell, so for
// every AO of the shell they read 64 consecutive doubles, and l (hence every loop bound below) is
// the same in all lanes.  The bracket has four weights per AO once the spin sum is taken,
//   W_0 = sum_s e_s (against d_x phi),  W_k = sum_s h_s(k) c_s (against d_x d_k phi), k = 1..3,
// and the block's four waves share them out: in GGA mode wave q takes weight q of the same 64
// points (a tile is 64 points), in LDA mode only W_0 exists and the four waves take four
// different groups of 64 points (a tile is 256 points).  A lane thus holds the 2l + 1 weights of
// one kind only.  The solid-harmonic transform is applied to the weights instead of to the
// derivatives, and the derivatives of one Cartesian component are formed in registers and
// consumed at once: no derivative plane exists anywhere.  The (l, q) bodies are templates, so
// the component loops unroll and the private arrays stay in registers.  In LDA mode h and c are
// not touched.
//
// Reduction without atomics: every wave sums its 64 lanes by shuffles, the four waves are added
// in order through LDS and the block writes partial[tile][shell][3]; k_gxc_tiles sums the tiles
// of a shell in ascending order, k_gxc_atoms folds the shells of an atom in table order into
// out.  Two calls on the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "xt_host.h"
#include "xt_internal.h"

namespace xt {

constexpr int kGxcBlock = 256;   // four waves

constexpr int gxc_ncart(int l) { return (l + 1) * (l + 2) / 2; }
constexpr int gxc_sph_off(int l) {   // start of the l table inside `sph`
  int o = 0;
  for (int k = 0; k < l; ++k) o += (2 * k + 1) * gxc_ncart(k);
  return o;
}

// One grid point g, one shell of angular momentum L and one weight Q (0: the first-derivative
// term, 1..3: the second-derivative term of direction k = Q): f[x] = that part of the bracket
// summed over the AOs of the shell and the spins.
template <int L, int Q>
__device__ __forceinline__ void gxc_shell(long g, const double* __restrict__ coords, int np,
                                          const double* __restrict__ ex, const double* __restrict__ sph,
                                          const double* __restrict__ norm, int ao0, int nao, int nspin,
                                          const double* __restrict__ h, const double* __restrict__ e,
                                          const double* __restrict__ c, long ldg, double (&f)[3]) {
  constexpr int NS = 2 * L + 1, NC = gxc_ncart(L), K = Q > 0 ? Q - 1 : 0;
  const double* cf = ex + np;
  const double* ctr = cf + np;
  const double r[3] = {coords[3 * g] - ctr[0], coords[3 * g + 1] - ctr[1], coords[3 * g + 2] - ctr[2]};
  const double r2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  // radial part R(r^2) = sum_k c_k exp(-a_k r^2): g0 = R, g1 = R' / r, g2 = (R' / r)' / r
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;
  for (int k = 0; k < np; ++k) {
    const double a2 = -2.0 * ex[k];
    const double v = cf[k] * exp(-ex[k] * r2);
    g0 += v;
    g1 += a2 * v;
    if (Q > 0) g2 += a2 * a2 * v;
  }
  // the spin-summed weights of the shell's AOs, AO norm included
  double W[NS];
#pragma unroll
  for (int m = 0; m < NS; ++m) {
    double w = 0.0;
    for (int s = 0; s < nspin; ++s) {
      const long row = ((long)s * nao + ao0 + m) * ldg + g;
      if (Q == 0)
        w += e[row];
      else
        w += h[(4 * (long)s + Q) * ldg + g] * c[row];
    }
    W[m] = norm[ao0 + m] * w;
  }
  double p[3][L + 1];   // powers r_d^0 .. r_d^L
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    p[d][0] = 1.0;
#pragma unroll
    for (int i = 1; i <= L; ++i) p[d][i] = p[d][i - 1] * r[d];
  }
  const double* T = sph + gxc_sph_off(L);
  double acc[3] = {0.0, 0.0, 0.0};
  int k = 0;
#pragma unroll
  for (int ix = L; ix >= 0; --ix) {
#pragma unroll
    for (int iy = L - ix; iy >= 0; --iy, ++k) {
      const int idx[3] = {ix, iy, L - ix - iy};
      // F0, F1, F2[d]: r_d^i and its first and second derivative (i is a constant after unrolling)
      double F0[3], F1[3], F2[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const int i = idx[d];
        F0[d] = p[d][i];
        F1[d] = i >= 1 ? i * p[d][i >= 1 ? i - 1 : 0] : 0.0;
        F2[d] = i >= 2 ? (i * (i - 1)) * p[d][i >= 2 ? i - 2 : 0] : 0.0;
      }
      const double P = F0[0] * F0[1] * F0[2];
      const double P1[3] = {F1[0] * F0[1] * F0[2], F0[0] * F1[1] * F0[2], F0[0] * F0[1] * F1[2]};
      // Cartesian weight of this component: sum_m T[m][k] W[m]
      double wc = 0.0;
#pragma unroll
      for (int m = 0; m < NS; ++m) wc += T[m * NC + k] * W[m];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double d;
        if (Q == 0) {
          d = P1[j] * g0 + P * g1 * r[j];
        } else {
          // d_j d_K (P R) = P_jK g0 + (P_j r_K + P_K r_j) g1 + P (delta_jK g1 + r_j r_K g2)
          const double PjK = j == K ? F2[K] * F0[(K + 1) % 3] * F0[(K + 2) % 3] : F1[j] * F1[K] * F0[3 - j - K];
          d = PjK * g0 + (P1[j] * r[K] + P1[K] * r[j]) * g1 + P * g2 * r[j] * r[K];
          if (j == K) d += P * g1;
        }
        acc[j] += d * wc;
      }
    }
  }
  f[0] = acc[0]; f[1] = acc[1]; f[2] = acc[2];
}

template <int LMAX, int Q>
__device__ __forceinline__ void gxc_any_l(int l, long g, const double* __restrict__ coords, int np,
                                          const double* __restrict__ ex, const double* __restrict__ sph,
                                          const double* __restrict__ norm, int ao0, int nao, int nspin,
                                          const double* __restrict__ h, const double* __restrict__ e,
                                          const double* __restrict__ c, long ldg, double (&f)[3]) {
#define XT_GXC(LL) \
  case LL: \
    if constexpr (LL <= LMAX) gxc_shell<LL, Q>(g, coords, np, ex, sph, norm, ao0, nao, nspin, h, e, c, ldg, f); \
    break
  switch (l) {
    XT_GXC(0);
    XT_GXC(1);
    XT_GXC(2);
    XT_GXC(3);
    XT_GXC(4);
  }
#undef XT_GXC
}

// block b = tile * nshell + shell; partial[3 b + x].  GGA: wave q of the block takes weight q of
// the tile's 64 points; LDA: the block's 256 lanes are 256 points.
template <bool GGA, int LMAX>
__global__ void __launch_bounds__(kGxcBlock)
k_grad_xc(int ngrid, const double* __restrict__ coords, int nshell, const int* __restrict__ shell_info,
          const double* __restrict__ dat, const double* __restrict__ sph, const double* __restrict__ norm,
          int lmax, int nao, int nspin, const double* __restrict__ h, const double* __restrict__ e,
          const double* __restrict__ c, long ldg, double* __restrict__ partial) {
  const int tile = blockIdx.x / nshell, s = blockIdx.x % nshell;
  const int* si = shell_info + 8 * (long)s;
  const int l = si[0], np = si[1], off = si[2], ao0 = si[3];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long g = GGA ? (long)tile * 64 + lane : (long)tile * kGxcBlock + threadIdx.x;
  // a shell above the declared bound or outside the AO range adds nothing
  const bool ok = l >= 0 && l <= lmax && l <= LMAX && np >= 0 && off >= 0 && ao0 >= 0 && ao0 + 2 * l + 1 <= nao;
  double f[3] = {0.0, 0.0, 0.0};
  if (ok && g < ngrid) {
    const double* ex = dat + off;
    if (!GGA || wave == 0)
      gxc_any_l<LMAX, 0>(l, g, coords, np, ex, sph, norm, ao0, nao, nspin, h, e, c, ldg, f);
    else if (wave == 1)
      gxc_any_l<LMAX, 1>(l, g, coords, np, ex, sph, norm, ao0, nao, nspin, h, e, c, ldg, f);
    else if (wave == 2)
      gxc_any_l<LMAX, 2>(l, g, coords, np, ex, sph, norm, ao0, nao, nspin, h, e, c, ldg, f);
    else
      gxc_any_l<LMAX, 3>(l, g, coords, np, ex, sph, norm, ao0, nao, nspin, h, e, c, ldg, f);
  }
  // the 64 lanes of a wave, then the waves in order
  __shared__ double red[kGxcBlock / 64][3];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    double v = f[m];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    f[m] = v;
  }
  if (lane == 0) {
    red[wave][0] = f[0];
    red[wave][1] = f[1];
    red[wave][2] = f[2];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = 0.0;
    for (int w = 0; w < kGxcBlock / 64; ++w) v += red[w][threadIdx.x];
    partial[3 * (long)blockIdx.x + threadIdx.x] = v;
  }
}

// ssum[s][m] = sum_t partial[t][s][m], t ascending
__global__ void k_gxc_tiles(int nshell, int ntile, const double* __restrict__ partial, double* __restrict__ ssum) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = 3 * (long)nshell;
  if (i >= n) return;
  double v = 0.0;
  for (int t = 0; t < ntile; ++t) v += partial[t * n + i];
  ssum[i] = v;
}

// out[A][m] += sum_{s: atom(s) = A} ssum[s][m], s ascending; one thread per (A, m)
__global__ void k_gxc_atoms(int nshell, int natm, const int* __restrict__ shell_atom,
                            const double* __restrict__ ssum, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * natm) return;
  const int A = i / 3, m = i % 3;
  double v = 0.0;
  for (int s = 0; s < nshell; ++s)
    if (shell_atom[s] == A) v += ssum[3 * (long)s + m];
  out[i] += v;
}

// grid points per block: 64 in GGA mode, 256 in LDA mode
static long gxc_tiles(int ngrid, bool gga) {
  const int t = gga ? 64 : kGxcBlock;
  return ((long)ngrid + t - 1) / t;
}

// doubles of workspace in either mode: the partial sums of every (tile, shell) at the GGA tile
// and the per-shell sums
long grad_xc_work(int ngrid, int nshell) { return 3 * (long)nshell * (gxc_tiles(ngrid, true) + 1); }

}  // namespace xt

using namespace xt;

extern "C" int xt_grad_xc(int ngrid, const double* coords, int nshell, const int* shell_info,
                          const double* shell_data, const double* sph, const double* ao_norm,
                          const int* shell_atom, int lmax, int natm, int nao, int nspin, int xctype,
                          const double* h, const double* e, const double* c, long ldg, double* work, long nwork,
                          double* out, void* stream) {
  if (ngrid < 0 || nshell < 0 || natm < 0 || nao < 0 || ldg < 0 || nwork < 0)
    return fail(XT_ERR_ARG, "xt_grad_xc: negative size");
  if (lmax < 0 || lmax > kAoMaxL) return fail(XT_ERR_ARG, "xt_grad_xc: lmax must be 0..4");
  if (nspin != 1 && nspin != 2) return fail(XT_ERR_ARG, "xt_grad_xc: nspin must be 1 or 2");
  if (xctype != XT_XC_LDA && xctype != XT_XC_GGA) return fail(XT_ERR_ARG, "xt_grad_xc: xctype must be XT_XC_LDA or XT_XC_GGA");
  if (ldg < ngrid) return fail(XT_ERR_ARG, "xt_grad_xc: ldg < ngrid");
  if (nwork < grad_xc_work(ngrid, nshell)) return fail(XT_ERR_ARG, "xt_grad_xc: workspace too small");
  const bool gga = xctype == XT_XC_GGA;
  const long nblock = gxc_tiles(ngrid, gga) * nshell;
  if (nblock > INT_MAX) return fail(XT_ERR_ARG, "xt_grad_xc: more than 2^31 (tile, shell) blocks, split the grid");
  if (nblock == 0 || natm == 0) return 0;
  if (!coords || !shell_info || !shell_data || !sph || !ao_norm || !shell_atom || !e || !work || !out)
    return fail(XT_ERR_ARG, "xt_grad_xc: null table, operand, workspace or output");
  if (gga && (!h || !c)) return fail(XT_ERR_ARG, "xt_grad_xc: the GGA term needs h and c");
  hipStream_t st = (hipStream_t)stream;
  const int ntile = (int)gxc_tiles(ngrid, gga);
  double* partial = work;
  double* ssum = work + 3 * nblock;
#define XT_GXC_RUN(G, LM)                                                                                  \
  hipLaunchKernelGGL((k_grad_xc<G, LM>), dim3((unsigned)nblock), dim3(kGxcBlock), 0, st, ngrid, coords, nshell, \
                     shell_info, shell_data, sph, ao_norm, lmax, nao, nspin, h, e, c, ldg, partial)
  // two register budgets: s p d tables (every double-zeta basis) and tables with f / g shells
  if (gga) {
    if (lmax <= 2) XT_GXC_RUN(true, 2); else XT_GXC_RUN(true, kAoMaxL);
  } else {
    if (lmax <= 2) XT_GXC_RUN(false, 2); else XT_GXC_RUN(false, kAoMaxL);
  }
#undef XT_GXC_RUN
  if (hipGetLastError() != hipSuccess) return fail(XT_ERR_HIP, "xt_grad_xc: launch failed");
  hipLaunchKernelGGL(k_gxc_tiles, dim3((unsigned)((3 * (long)nshell + 63) / 64)), dim3(64), 0, st, nshell, ntile,
                     partial, ssum);
  hipLaunchKernelGGL(k_gxc_atoms, dim3((unsigned)((3 * natm + 63) / 64)), dim3(64), 0, st, nshell, natm,
                     shell_atom, ssum, out);
  return hipGetLastError() == hipSuccess ? 0 : fail(XT_ERR_HIP, "xt_grad_xc: launch failed");
}
