// Coulomb integrals between charge distributions given directly in Hermite form -- the
// derivative integrals of the spin-orbit mean field (xtddft_amd/somf.py; the reference's
// sfX2C_soDKH1.py get_kint / get_wso / int1e_pnucp, there libcint's int2e_ip1ip2,
// cint1e_prinvxp and int1e_pnucp).
//
// A differentiated Gaussian pair is a Hermite expansion one order higher per derivative
// (qc/ints.py deriv_tables), so the McMurchie-Davidson quartic part of xt_int.hip applies
// unchanged; what differs from k_int_cart is that a table entry states its Hermite order and
// its number of component rows instead of implying both by (la, lb):
//
//   bra_info[8 k + .]: order, nrow, npp, prim0, e0, row0, tag;  bra_prim[4 q + .]: p, Px, Py, Pz
//   ket_info[8 j + .]: order, nprim, prim0, e0, col0, ncol, tag; ket_prim[4 r + .]: s, Cx, Cy, Cz
//   eb (bra k): [row][t][q] over nrow x ntuv(order) x npp;  ek (ket j): [col][u][r]
//
//   plain: out[(row0 + row) ldo + col0 + col] += (row | col)
//   cross: the rows are (m, ab) and the columns (n, cd), m, n = x, y, z outermost (nrow = 3 nab,
//          ncol = 3 ncd); out[(l nrow_tot + row0 + ab) ldo + col0 + cd] += eps_lmn ((m, ab) | (n, cd)):
//          K^l = eps_lmn (d_m a  b | d_n c  d) of get_kint.  The three m = n products are not formed.
//
// A quartet whose bra and ket tags differ is skipped (its block stays zero): the one-centre
// approximation tags every same-atom pair with its atom, and all atoms share the launches.
//
// One thread per (bra entry, ket entry), the bra index fastest over entries the caller orders
// by class (qc/dints.py DerivPairTable), as k_int_cart.  Point charges as kets of order 0 and
// infinite exponent give the one-electron integrals (qc/dints.py int1e_pvp_device).
//
// Total order up to 14 ((d f  f | d f  f)), one above xt_int.hip's kIntMaxL: the Boys table for
// orders up to 14 + 6 and the R_tuv recursion live in xt_hint_dev.h (shared with xt_grad.hip) and
// leave xt_int.hip's table and kernels as they are.
#include <hip/hip_runtime.h>
#include <math.h>
#include "xt_internal.h"
#include "xt_hermite.h"
#include "xt_hint_dev.h"

namespace xt {

// MAXL: largest total order, MAXLB: largest bra order (they size R / S and M)
template <int MAXL, int MAXLB>
__global__ void __launch_bounds__(64)
k_hint_cart(int nbra, const int* __restrict__ bra_info, const double* __restrict__ bra_prim,
            const double* __restrict__ eb, int nket, const int* __restrict__ ket_info,
            const double* __restrict__ ket_prim, const double* __restrict__ ek, int cross, long nrow_tot,
            double* __restrict__ out, long ldo) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)nbra * nket) return;
  const int j = (int)(id / nbra), k = (int)(id % nbra);
  const int* bi = bra_info + 8 * k;
  const int* ki = ket_info + 8 * j;
  const int lb = bi[0], nrow = bi[1], npp = bi[2], bq0 = bi[3], be0 = bi[4], row0 = bi[5];
  const int lk = ki[0], nr = ki[1], kr0 = ki[2], ke0 = ki[3], col0 = ki[4], ncol = ki[5];
  if (bi[6] != ki[6]) return;
  const int L = lb + lk, ntb = ntuv(lb), ntk = ntuv(lk);
  if (L > MAXL || lb > MAXLB) return;   // an entry above the declared bounds: left as the caller's zeros
  const int nab = cross ? nrow / 3 : nrow, ncd = cross ? ncol / 3 : ncol;
  double R[ntuv(MAXL)], S[ntuv(MAXL)], M[ntuv(MAXLB)];
  for (int q = 0; q < npp; ++q) {
    const double* pp = bra_prim + 4 * (long)(bq0 + q);
    const double p = pp[0];
    for (int r = 0; r < nr; ++r) {
      const double* cp = ket_prim + 4 * (long)(kr0 + r);
      const double s = cp[0];
      hint_r<MAXL>(L, p * s / (p + s), pp[1] - cp[1], pp[2] - cp[2], pp[3] - cp[3], R, S);
      const double pref = 2.0 * pow(M_PI, 2.5) / (p * s * sqrt(p + s));
      for (int c = 0; c < ncol; ++c) {
        // M[t] = sum_u (-1)^{|u|} E^c_u(r) R[t + u]
        const double* e = ek + ke0 + ((long)c * ntk) * nr + r;
        for (int it = 0; it < ntb; ++it) M[it] = 0.0;
        int iu = 0;
        for (int nu = 0; nu <= lk; ++nu)
          for (int tu = nu; tu >= 0; --tu)
            for (int uu = nu - tu; uu >= 0; --uu, ++iu) {
              const int vu = nu - tu - uu;
              const double w = ((nu & 1) ? -1.0 : 1.0) * e[(long)iu * nr];
              if (w == 0.0) continue;
              int it = 0;
              for (int nt = 0; nt <= lb; ++nt)
                for (int tt = nt; tt >= 0; --tt)
                  for (int ut = nt - tt; ut >= 0; --ut, ++it)
                    M[it] += w * R[tuv_pos(tt + tu, ut + uu, nt - tt - ut + vu)];
            }
        const int n = cross ? c / ncd : 0, cd = c - n * ncd;
        for (int row = 0; row < nrow; ++row) {
          const int m = cross ? row / nab : 0;
          if (cross && m == n) continue;
          const double* ea = eb + be0 + ((long)row * ntb) * npp + q;
          double acc = 0.0;
          for (int it = 0; it < ntb; ++it) acc += ea[(long)it * npp] * M[it];
          if (cross) {   // eps_lmn: l = 3 - m - n, +1 when n follows m cyclically
            const int l = 3 - m - n;
            const double sg = (n == (m + 1) % 3) ? 1.0 : -1.0;
            out[((long)l * nrow_tot + row0 + (row - m * nab)) * ldo + col0 + cd] += sg * pref * acc;
          } else {
            out[(long)(row0 + row) * ldo + col0 + c] += pref * acc;
          }
        }
      }
    }
  }
}

int hint_cart(int nbra, const int* bra_info, const double* bra_prim, const double* eb, int nket,
              const int* ket_info, const double* ket_prim, const double* ek, int lbra, int lket, int cross,
              long nrow_tot, double* out, long ldo, hipStream_t st) {
  const long n = (long)nbra * nket;
  if (n == 0) return 0;
  if (hint_boys_ensure(st)) return XT_ERR_HIP;   // the Boys table, once per device
  const int blk = 64;
  const dim3 grid((unsigned)((n + blk - 1) / blk));
#define XT_HINT(ML, MB)                                                                                    \
  hipLaunchKernelGGL((k_hint_cart<ML, MB>), grid, dim3(blk), 0, st, nbra, bra_info, bra_prim, eb, nket, \
                     ket_info, ket_prim, ek, cross, nrow_tot, out, ldo)
  if (lbra <= 4 && lbra + lket <= 6)   // s, p shells: (d a b | d c d) 3 + 3, (d a d b | C) 4 + 0
    XT_HINT(6, 4);
  else if (lbra <= 6 && lbra + lket <= 10)   // d shells
    XT_HINT(10, 6);
  else if (lbra <= kHintMaxLBra && lbra + lket <= kHintMaxL)   // f shells
    XT_HINT(kHintMaxL, kHintMaxLBra);
  else
    return XT_ERR_ARG;
#undef XT_HINT
  return hipGetLastError() == hipSuccess ? 0 : XT_ERR_HIP;
}

}  // namespace xt
