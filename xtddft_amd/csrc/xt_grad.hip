// First-derivative Coulomb integrals contracted with a two-particle density straight to a force
// on the atoms -- the two-electron part of every analytic nuclear gradient (xtddft_amd/qc/grad.py,
// xtddft_amd/grad.py; the reference's grad_jp/grad/usfcis.py, there PySCF's get_jk / get_k over
// libcint's int2e_ip1):
//
//   g[A][m] = sum_{a in A} sum_{b,c,d} (d_m a  b | c d) Gamma_abcd,      m = x, y, z
//   Gamma_abcd = sum_{t < nterm} wj[t] P_t[a,b] Q_t[c,d] + wk[t] P_t[a,c] Q_t[b,d]           (xt_grad_jk)
//   Gamma_abcd = sum_{t < nj} wj[t] PJ_t[a,b] QJ_t[c,d] + sum_{t < nk} wk[t] PK_t[a,c] QK_t[b,d]   (xt_grad_jk2)
//
//   the same Gamma with (d_m a b | c d) over erf(omega r12) / r12                                 (xt_grad_jk2_lr)
//
// One kernel body serves all three: k_grad_jk is a template over the functor that forms Gamma and over
// the operator (Coulomb: 1/r12; ErfLR: the long-range part of a range-separated hybrid's exchange).
//
// d_m a is what the bra table holds (qc/ints.py deriv_tables: the derivative with respect to the
// centre of a, the negative of the electron-coordinate derivative; the host fixes the sign);
// P_t, Q_t are arbitrary (not necessarily symmetric) matrices over Cartesian components.  The integrals are k_hint_cart's
// (xt_hint.hip): the bra is an ordered DerivPair entry (rows (m, ca, cb), order la + lb + 1), the
// ket a plain shell pair c >= d of the pair table; where k_hint_cart stores pref * acc, this
// kernel multiplies it by its Gamma element and adds it to one of three sums, so no integral
// reaches HBM.  For c != d the thread adds the (d, c) image of Gamma itself: (ab|cd) = (ab|dc).
//
//   bra_info / bra_prim / eb, ket_info / ket_prim / ek: as xt_hint_cart (row0 / col0 unused)
//   bra_ao[4 k + .]: first Cartesian AO of a, of b, ncart(b), atom of a
//   ket_ao[4 j + .]: first Cartesian AO of c, of d, ncart(d), 1 when c != d (add the image)
//
// Reduction without atomics: a thread owns one bra entry and a strip of at most `strip` ket entries
// (strip s takes the entries s, s + nstrip, ...: the table is sorted by primitive count, and consecutive
// entries would put all the long quartets into the first strips) and writes partial[strip][bra][3];
// k_grad_strips sums the strips of a bra entry in
// strip order, k_grad_atoms folds the bra entries into their atoms in table order.  Two calls on
// the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include "xt_internal.h"
#include "xt_hermite.h"
#include "xt_hint_dev.h"

namespace xt {

struct GradTerms {
  int nterm;
  double wj[kGradMaxTerms], wk[kGradMaxTerms];
};

// Gamma of one (bra block, ket block) is kept per thread when it has at most this many elements
// (every s / p quartet: 9 x 9); larger blocks recompute the element per primitive quartet
constexpr int kGradCache = 81;

// How Gamma_abcd is formed: k_grad_jk is a template over one of these.  GammaPairs is xt_grad_jk's
// (every pair carries a Coulomb and an exchange weight), GammaLists xt_grad_jk2's (a Coulomb list
// and an exchange list of their own, so that a pair costs one product, not two).
struct GammaPairs {
  GradTerms tm;
  const double* __restrict__ P;
  const double* __restrict__ Q;
  __device__ __forceinline__ double operator()(long n, long ia, long ib, long ic, long id) const {
    double g = 0.0;
    const long n2 = n * n;
    for (int t = 0; t < tm.nterm; ++t) {
      const double* p = P + t * n2;
      const double* q = Q + t * n2;
      g += tm.wj[t] * p[ia * n + ib] * q[ic * n + id] + tm.wk[t] * p[ia * n + ic] * q[ib * n + id];
    }
    return g;
  }
};

struct GammaLists {
  int nj, nk;
  double wj[kGradMaxTerms], wk[kGradMaxTerms];
  const double* __restrict__ PJ;
  const double* __restrict__ QJ;
  const double* __restrict__ PK;
  const double* __restrict__ QK;
  __device__ __forceinline__ double operator()(long n, long ia, long ib, long ic, long id) const {
    double g = 0.0;
    const long n2 = n * n;
    for (int t = 0; t < nj; ++t) g += wj[t] * PJ[t * n2 + ia * n + ib] * QJ[t * n2 + ic * n + id];
    for (int t = 0; t < nk; ++t) g += wk[t] * PK[t * n2 + ia * n + ic] * QK[t * n2 + ib * n + id];
    return g;
  }
};

// The operator of the integrals, a compile-time parameter of k_grad_jk.  Coulomb is 1/r12 and holds
// nothing: its instantiations are the kernel without any of the lines below `if constexpr`.  ErfLR is
// erf(omega r12) / r12 by the formula of xt_int.hip (qc/ints.py _attenuate): per primitive quartet with
// alpha = p s / (p + s), the Hermite integrals at a2 = alpha w^2 / (alpha + w^2) times sqrt(a2 / alpha).
struct Coulomb {
  static constexpr bool kAttenuated = false;
};
struct ErfLR {
  static constexpr bool kAttenuated = true;
  double w2;   // omega^2
};
// What the kernel takes by value: the Gamma functor and the operator's data in one argument.  Coulomb is
// an empty base, so GradArgs<Gamma, Coulomb> has the layout of Gamma and the 1/r12 instantiations keep
// their kernel arguments as they were.
template <class Gamma, class Op>
struct GradArgs : Gamma, Op {};

// MAXL: largest total order, MAXLB: largest bra order (they size R / S and M)
template <int MAXL, int MAXLB, class Gamma, class Op>
__global__ void __launch_bounds__(64)
k_grad_jk(int nbra, const int* __restrict__ bra_info, const double* __restrict__ bra_prim,
          const double* __restrict__ eb, const int* __restrict__ bra_ao, int nket,
          const int* __restrict__ ket_info, const double* __restrict__ ket_prim, const double* __restrict__ ek,
          const int* __restrict__ ket_ao, GradArgs<Gamma, Op> gm, long nao, int nstrip, double* __restrict__ partial) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)nbra * nstrip) return;
  const int s = (int)(id / nbra), k = (int)(id % nbra);
  const int* bi = bra_info + 8 * k;
  const int lb = bi[0], nrow = bi[1], npp = bi[2], bq0 = bi[3], be0 = bi[4];
  const int a0 = bra_ao[4 * k], b0 = bra_ao[4 * k + 1], ncb = bra_ao[4 * k + 2] > 0 ? bra_ao[4 * k + 2] : 1;
  const int nab = nrow / 3, ntb = ntuv(lb);
  double g[3] = {0.0, 0.0, 0.0};
  double R[ntuv(MAXL)], S[ntuv(MAXL)], M[ntuv(MAXLB)], G[kGradCache];
  for (int j = s; j < nket; j += nstrip) {   // at most `strip` entries
    const int* ki = ket_info + 8 * j;
    const int lk = ki[0], nr = ki[1], kr0 = ki[2], ke0 = ki[3], ncol = ki[5];
    const int c0 = ket_ao[4 * j], d0 = ket_ao[4 * j + 1], image = ket_ao[4 * j + 3];
    const int ncd = ket_ao[4 * j + 2] > 0 ? ket_ao[4 * j + 2] : 1;
    const int L = lb + lk, ntk = ntuv(lk);
    if (L > MAXL || lb > MAXLB) continue;   // an entry above the declared bounds adds nothing
    const bool cached = nab * ncol <= kGradCache;
    if (cached)
      for (int c = 0; c < ncol; ++c) {
        const long ic = c0 + c / ncd, idd = d0 + c % ncd;
        for (int ab = 0; ab < nab; ++ab) {
          const long ia = a0 + ab / ncb, ib = b0 + ab % ncb;
          double v = gm(nao, ia, ib, ic, idd);
          if (image) v += gm(nao, ia, ib, idd, ic);
          G[c * nab + ab] = v;
        }
      }
    for (int q = 0; q < npp; ++q) {
      const double* pp = bra_prim + 4 * (long)(bq0 + q);
      const double p = pp[0];
      for (int r = 0; r < nr; ++r) {
        const double* cp = ket_prim + 4 * (long)(kr0 + r);
        const double sx = cp[0];
        double alpha = p * sx / (p + sx);
        if constexpr (Op::kAttenuated) alpha = alpha * gm.w2 / (alpha + gm.w2);   // a2
        hint_r<MAXL>(L, alpha, pp[1] - cp[1], pp[2] - cp[2], pp[3] - cp[3], R, S);
        double pref = 2.0 * pow(M_PI, 2.5) / (p * sx * sqrt(p + sx));
        // the R's times sqrt(a2 / alpha) = sqrt(w^2 / (alpha + w^2)), through pref (R enters linearly);
        // formed after hint_r so that nothing more is live across it
        if constexpr (Op::kAttenuated) pref *= sqrt(gm.w2 / (p * sx / (p + sx) + gm.w2));
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
          const long ic = c0 + c / ncd, idd = d0 + c % ncd;
          for (int ab = 0; ab < nab; ++ab) {
            double gam;
            if (cached) {
              gam = G[c * nab + ab];
            } else {
              const long ia = a0 + ab / ncb, ib = b0 + ab % ncb;
              gam = gm(nao, ia, ib, ic, idd);
              if (image) gam += gm(nao, ia, ib, idd, ic);
            }
            gam *= pref;
            for (int m = 0; m < 3; ++m) {
              const double* ea = eb + be0 + ((long)(m * nab + ab) * ntb) * npp + q;
              double acc = 0.0;
              for (int it = 0; it < ntb; ++it) acc += ea[(long)it * npp] * M[it];
              g[m] += gam * acc;
            }
          }
        }
      }
    }
  }
  double* out = partial + 3 * ((long)s * nbra + k);
  out[0] = g[0]; out[1] = g[1]; out[2] = g[2];
}

// bsum[k][m] = sum_s partial[s][k][m], s ascending
__global__ void k_grad_strips(int nbra, int nstrip, const double* __restrict__ partial, double* __restrict__ bsum) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = 3 * (long)nbra;
  if (i >= n) return;
  double v = 0.0;
  for (int s = 0; s < nstrip; ++s) v += partial[s * n + i];
  bsum[i] = v;
}

// out[A][m] += sum_{k: atom(k) = A} bsum[k][m], k ascending; one thread per (A, m)
__global__ void k_grad_atoms(int nbra, int natm, const int* __restrict__ bra_ao, const double* __restrict__ bsum,
                             double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * natm) return;
  const int A = i / 3, m = i % 3;
  double v = 0.0;
  for (int k = 0; k < nbra; ++k)
    if (bra_ao[4 * k + 3] == A) v += bsum[3 * (long)k + m];
  out[i] += v;
}

long grad_jk_work(int nbra, int nket, int strip) {
  const long nstrip = ((long)nket + strip - 1) / strip;
  return 3 * (long)nbra * (nstrip + 1);
}

// the three launches of one call, for either way of forming Gamma and either operator
template <class Gamma, class Op>
static int grad_launch(int nbra, const int* bra_info, const double* bra_prim, const double* eb, const int* bra_ao,
                       int nket, const int* ket_info, const double* ket_prim, const double* ek, const int* ket_ao,
                       int lbra, int lket, const Gamma& gm, long nao, int strip, int natm, double* work,
                       double* out, hipStream_t st, const Op& op) {
  if (hint_boys_ensure(st)) return XT_ERR_HIP;
  const int nstrip = (int)(((long)nket + strip - 1) / strip);   // <= nket
  const long n = (long)nbra * nstrip;
  double* partial = work;
  double* bsum = work + 3 * n;
  const int blk = 64;
  const dim3 grid((unsigned)((n + blk - 1) / blk));
  const GradArgs<Gamma, Op> ga{gm, op};
#define XT_GRAD(ML, MB)                                                                                   \
  hipLaunchKernelGGL((k_grad_jk<ML, MB, Gamma, Op>), grid, dim3(blk), 0, st, nbra, bra_info, bra_prim,  \
                     eb, bra_ao, nket, ket_info, ket_prim, ek, ket_ao, ga, nao, nstrip, partial)
  if (lbra <= 4 && lbra + lket <= 6)   // s, p shells: (d p p | p p) 3 + 2
    XT_GRAD(6, 4);
  else if (lbra <= 6 && lbra + lket <= 10)   // d shells: (d d d | d d) 5 + 4
    XT_GRAD(10, 6);
  else if (lbra <= kHintMaxLBra && lbra + lket <= kHintMaxL)   // f shells: (d f f | f f) 7 + 6
    XT_GRAD(kHintMaxL, kHintMaxLBra);
  else
    return XT_ERR_ARG;
#undef XT_GRAD
  if (hipGetLastError() != hipSuccess) return XT_ERR_HIP;
  hipLaunchKernelGGL(k_grad_strips, dim3((unsigned)((3 * (long)nbra + 63) / 64)), dim3(64), 0, st, nbra, nstrip,
                     partial, bsum);
  hipLaunchKernelGGL(k_grad_atoms, dim3((unsigned)((3 * natm + 63) / 64)), dim3(64), 0, st, nbra, natm, bra_ao,
                     bsum, out);
  return hipGetLastError() == hipSuccess ? 0 : XT_ERR_HIP;
}

int grad_jk(int nbra, const int* bra_info, const double* bra_prim, const double* eb, const int* bra_ao, int nket,
            const int* ket_info, const double* ket_prim, const double* ek, const int* ket_ao, int lbra, int lket,
            int nterm, const double* wj, const double* wk, const double* P, const double* Q, long nao, int strip,
            int natm, double* work, double* out, hipStream_t st) {
  if (nbra == 0 || nket == 0 || natm == 0) return 0;
  GammaPairs gm;
  gm.tm.nterm = nterm;
  for (int t = 0; t < kGradMaxTerms; ++t) {
    gm.tm.wj[t] = t < nterm ? wj[t] : 0.0;
    gm.tm.wk[t] = t < nterm ? wk[t] : 0.0;
  }
  gm.P = P;
  gm.Q = Q;
  return grad_launch(nbra, bra_info, bra_prim, eb, bra_ao, nket, ket_info, ket_prim, ek, ket_ao, lbra, lket, gm, nao,
                     strip, natm, work, out, st, Coulomb{});
}

// omega == 0: 1/r12 (xt_grad_jk2); omega > 0: erf(omega r12) / r12 (xt_grad_jk2_lr)
int grad_jk2(int nbra, const int* bra_info, const double* bra_prim, const double* eb, const int* bra_ao, int nket,
             const int* ket_info, const double* ket_prim, const double* ek, const int* ket_ao, int lbra, int lket,
             int nj, const double* wj, const double* PJ, const double* QJ, int nk, const double* wk,
             const double* PK, const double* QK, long nao, int strip, int natm, double* work, double* out,
             hipStream_t st, double omega) {
  if (nbra == 0 || nket == 0 || natm == 0) return 0;
  GammaLists gm;
  gm.nj = nj;
  gm.nk = nk;
  for (int t = 0; t < kGradMaxTerms; ++t) {
    gm.wj[t] = t < nj ? wj[t] : 0.0;
    gm.wk[t] = t < nk ? wk[t] : 0.0;
  }
  gm.PJ = nj ? PJ : nullptr;   // an empty list is never read
  gm.QJ = nj ? QJ : nullptr;
  gm.PK = nk ? PK : nullptr;
  gm.QK = nk ? QK : nullptr;
  if (omega > 0.0)
    return grad_launch(nbra, bra_info, bra_prim, eb, bra_ao, nket, ket_info, ket_prim, ek, ket_ao, lbra, lket, gm,
                       nao, strip, natm, work, out, st, ErfLR{omega * omega});
  return grad_launch(nbra, bra_info, bra_prim, eb, bra_ao, nket, ket_info, ket_prim, ek, ket_ao, lbra, lket, gm, nao,
                     strip, natm, work, out, st, Coulomb{});
}

}  // namespace xt
