// xt_stda: the simplified open-shell TDA (sX-TDA / sU-TDA) of xtddft/sTDA/os_sTDA.py on the
// device (include/xtddft_amd.h): Loewdin atomic charges of orbital pairs, their gamma-contracted
// partners, and the three consumers of one element generator -- the diagonal (iaia_f,
// os_sTDA.py:33-44), the perturbative selection weights (iajb_f, :235-260, :752-793) and the
// dense A matrix of a CSF list (cAcvacva / cAcvacvb / cAcvbcvb and the block loops, :263-350,
// :1014-1221).
//
// Operand layout is pair-major: the natm charges of one orbital pair are contiguous,
//   q_ov[(i nvir + a) natm + A],  q_oo[(i nocc + j) natm + A],  q_vv[(a nvir + b) natm + A],
// so a CSF (s, i, a) owns one contiguous natm-vector of q_ov[s] and of gammaK q_ov[s], and a pair
// of CSFs of one spin owns one of q_oo[s] and one of gammaJ q_vv[s].
//
// Generator, one wave per 16 x 16 tile of (row CSF p, column CSF q):
//   line 1  K[p,q] = sum_A q_ov[p][A] (gammaK q_ov)[q][A]: v_mfma_f64_16x16x4 over the atom index,
//           natm zero-padded to a multiple of 4 by the load predicate; lane (k4, r) feeds row /
//           column r at atom 4 step + k4 straight from global memory (gathered, no LDS);
//   line 2  J[p,q] = sum_A q_oo[i_p,i_q][A] (gammaJ q_vv)[a_p,a_q][A], same spin only: both operands
//           depend on the pair, so every lane runs the natm-long dot product of each of its four
//           elements (rows k4 + 4 t, column r) in atom order.  The 64 gammaJ q_vv vectors of a step
//           are fetched by the whole wave (16 lanes along each contiguous vector, 16 atoms at a
//           time) and handed to their lanes through 8.5 KiB of wave-private LDS (pitch 17: the
//           per-lane reads hit distinct banks); the q_oo vectors, few per tile when the lists are
//           ordered by class and occupied index as the driver's are, are read directly;
//   Fock / X / correction: scalar epilogue.
// Every sum has one fixed order (the MFMA chain over atom steps, the J loop over atoms, the
// selection's loop over P tiles and its four-row fold), so two calls return the same bits; the
// diagonal entry runs the very same tile code on the diagonal tiles and returns the bits of
// xt_stda_matrix's diagonal.  No atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include "xt_host.h"

using namespace xt;

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

struct Gen {
  int natm;
  int nocc[2], nvir[2];
  int nc, no, nv;
  int sa;                 // X term active (spin_adapted and no > 0)
  double c1, c2, c3;
  int correct;
  double dmax, sigk;
  const double *qov[2], *kov[2], *qoo[2], *jvv[2], *foo[2], *fvv[2], *hoo[2], *hvv[2];
};

constexpr int JCH = 16;            // atoms per staged chunk of line 2
constexpr int JP = JCH + 1;        // LDS pitch of one element's chunk (odd: conflict-free reads)
constexpr int JLDS = 64 * JP;      // doubles of wave-private LDS

__device__ __forceinline__ void wave_sync() {   // orders this wave's LDS writes and reads across lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The 16 x 16 tile (rows r0.., columns c0..) of the generator for this wave.  Lane (k4, r) =
// (lane / 16, lane % 16) ends up with the elements (r0 + k4 + 4 t, c0 + r), t < 4: tot[t] the
// element, kl[t] its first line alone.  FULL: all five lines (same = the two lists are one list,
// so that "p = q" is "row = column"); otherwise the first two (the selection's B).  DIAG: only
// the elements with row = column are finished (the rest stay 0).  sj: JLDS doubles of LDS owned
// by this wave.  Every lane of the wave must call (MFMA, shuffles, the wave-level LDS staging).
template <bool FULL, bool DIAG>
__device__ __forceinline__ void gen_tile(const Gen& g, const int* __restrict__ rl, int nR, int r0,
                                         const int* __restrict__ cl, int nC, int c0, double* sj, double tot[4],
                                         double kl[4]) {
  const int lane = threadIdx.x & 63, k4 = lane >> 4, r = lane & 15;
  const int natm = g.natm;
  const double* pa = nullptr;
  const double* pb = nullptr;
  if (r0 + r < nR) {
    const int* e = rl + 3L * (r0 + r);
    pa = g.qov[e[0]] + ((long)e[1] * g.nvir[e[0]] + e[2]) * natm;
  }
  int sq = 0, iq = 0, aq = 0;
  const bool cok = c0 + r < nC;
  if (cok) {
    const int* e = cl + 3L * (c0 + r);
    sq = e[0]; iq = e[1]; aq = e[2];
    pb = g.kov[sq] + ((long)iq * g.nvir[sq] + aq) * natm;
  }
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < natm; k0 += 4) {
    const int k = k0 + k4;
    const double av = (pa && k < natm) ? pa[k] : 0.0;
    const double bv = (pb && k < natm) ? pb[k] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    // step t: the 64 elements (rows 4 t .. 4 t + 3) x (16 columns), element number = lane number
    const int row = r0 + k4 + 4 * t;
    const bool live = cok && row < nR && (!DIAG || row == c0 + r);
    int sp = 0, ip = 0, ap = 0;
    if (live) {
      const int* e = rl + 3L * row;
      sp = e[0]; ip = e[1]; ap = e[2];
    }
    const bool same = live && sp == sq;
    double j = 0.0;
    if (__ballot(same) != 0) {   // wave-uniform
      // line 2.  An element's gammaJ q_vv vector is natm contiguous doubles, so the wave fetches the
      // 64 vectors of this step together: chunk by chunk of JCH atoms, 16 lanes per vector and four
      // vectors per load instruction (whole cache lines), through LDS to the lane that owns the
      // element.  The q_oo vector is shared by the lanes with the same (i_p, i_q) and read directly.
      const double* x = nullptr;
      unsigned long long yp = 0;
      if (same) {
        x = g.qoo[sp] + ((long)ip * g.nocc[sp] + iq) * natm;
        yp = (unsigned long long)(g.jvv[sp] + ((long)ap * g.nvir[sp] + aq) * natm);
      }
      const unsigned ylo = (unsigned)yp, yhi = (unsigned)(yp >> 32);
      const double* ye[16];
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int e = 4 * jj + k4;
        const unsigned lo = (unsigned)__shfl((int)ylo, e), hi = (unsigned)__shfl((int)yhi, e);
        ye[jj] = (const double*)(((unsigned long long)hi << 32) | lo);
      }
      for (int a0 = 0; a0 < natm; a0 += JCH) {
        const int a = a0 + r;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj)
          sj[(4 * jj + k4) * JP + r] = (ye[jj] && a < natm) ? ye[jj][a] : 0.0;
        wave_sync();
        if (same) {
          const int na = natm - a0 < JCH ? natm - a0 : JCH;
          const double* y = sj + lane * JP;
          for (int b = 0; b < na; ++b) j += x[a0 + b] * y[b];   // atom order, as one loop over natm
        }
        wave_sync();
      }
    }
    tot[t] = 0.0;
    kl[t] = 0.0;
    if (!live) continue;
    const double kk = acc[t];
    double v = kk;
    if (sp == sq) {
      const int s = sp, no_s = g.nocc[s], nv_s = g.nvir[s];
      v -= j;
      if (FULL) {
        if (ip == iq) v += g.fvv[s][(long)ap * nv_s + aq];
        if (ap == aq) v -= g.foo[s][(long)ip * no_s + iq];
      }
    }
    if (FULL) {
      if (g.sa) {
        // CV(aa): alpha, core occupied; CV(bb): beta, virtual beyond the open shells
        const bool cvp = sp == 0 ? ip < g.nc : ap >= g.no;
        const bool cvq = sq == 0 ? iq < g.nc : aq >= g.no;
        if (cvp && cvq) {
          const int vp = sp == 0 ? ap : ap - g.no, vq = sq == 0 ? aq : aq - g.no;   // alpha virtual index
          double cij, cab;
          if (sp != sq) { cij = g.c3; cab = g.c3; }
          else if (sp == 0) { cij = g.c1; cab = g.c2; }
          else { cij = g.c2; cab = g.c1; }
          if (ip == iq)
            v += cij * (g.hvv[1][(long)(g.no + vp) * g.nvir[1] + g.no + vq] - g.hvv[0][(long)vp * g.nvir[0] + vq]);
          if (vp == vq)
            v += cab * (g.hoo[1][(long)ip * g.nocc[1] + iq] - g.hoo[0][(long)ip * g.nocc[0] + iq]);
        }
      }
      if (g.correct && row == c0 + r) {
        const double x = kk / g.sigk, x2 = x * x;
        v += g.dmax / (1.0 + x2 * x2);
      }
    }
    tot[t] = v;
    kl[t] = kk;
  }
}

// A (n x n): one wave per tile, four waves per block
__global__ __launch_bounds__(256) void k_stda_matrix(Gen g, const int* __restrict__ csf, int n, int nt,
                                                     double* __restrict__ out) {
  __shared__ double sj[4][JLDS];
  const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= (long)nt * nt) return;   // wave-uniform
  const int r0 = (int)(tile / nt) * 16, c0 = (int)(tile % nt) * 16;
  double tot[4], kl[4];
  gen_tile<true, false>(g, csf, n, r0, csf, n, c0, sj[threadIdx.x >> 6], tot, kl);
  const int lane = threadIdx.x & 63, k4 = lane >> 4, r = lane & 15;
  if (c0 + r >= n) return;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = r0 + k4 + 4 * t;
    if (row < n) out[(long)row * n + c0 + r] = tot[t];
  }
}

// E_p = A[p,p] and K_pp: the diagonal tiles of the same generator
__global__ __launch_bounds__(256) void k_stda_diag(Gen g, const int* __restrict__ csf, int n, int nt,
                                                   double* __restrict__ e, double* __restrict__ kpp) {
  __shared__ double sj[4][JLDS];
  const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= nt) return;   // wave-uniform
  const int r0 = (int)tile * 16;
  double tot[4], kl[4];
  gen_tile<true, true>(g, csf, n, r0, csf, n, r0, sj[threadIdx.x >> 6], tot, kl);
  const int lane = threadIdx.x & 63, k4 = lane >> 4, r = lane & 15;
  if (r0 + r >= n || (r & 3) != k4) return;
  const int t = r >> 2;   // row k4 + 4 t = r
  const double ev = t == 0 ? tot[0] : t == 1 ? tot[1] : t == 2 ? tot[2] : tot[3];
  const double kv = t == 0 ? kl[0] : t == 1 ? kl[1] : t == 2 ? kl[2] : kl[3];
  e[r0 + r] = ev;
  if (kpp) kpp[r0 + r] = kv;
}

// w_q = sum_p B[p,q]^2 / (E_q - E_p + 1e-10): one wave per 16 columns of N, the P tiles in order;
// a lane sums its rows k4 + 4 t of every tile, then the four row groups fold in the order k4 = 0..3
__global__ __launch_bounds__(256) void k_stda_select(Gen g, const int* __restrict__ pl, int nP,
                                                     const double* __restrict__ eP, const int* __restrict__ nl, int nN,
                                                     const double* __restrict__ eN, int nt, double* __restrict__ w) {
  __shared__ double sj[4][JLDS];
  const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= nt) return;   // wave-uniform
  const int c0 = (int)tile * 16;
  const int lane = threadIdx.x & 63, k4 = lane >> 4, r = lane & 15;
  const bool cok = c0 + r < nN;
  const double eq = cok ? eN[c0 + r] : 0.0;
  double sum = 0.0;
  for (int r0 = 0; r0 < nP; r0 += 16) {
    double tot[4], kl[4];
    gen_tile<false, false>(g, pl, nP, r0, nl, nN, c0, sj[threadIdx.x >> 6], tot, kl);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int row = r0 + k4 + 4 * t;
      if (cok && row < nP) sum += tot[t] * tot[t] / (eq - eP[row] + 1e-10);
    }
  }
  const double s0 = __shfl(sum, r), s1 = __shfl(sum, r + 16), s2 = __shfl(sum, r + 32), s3 = __shfl(sum, r + 48);
  if (cok && k4 == 0) w[c0 + r] = ((s0 + s1) + s2) + s3;
}

// out[(p nq + q) natm + A] = sum_{mu in atom A} C[mu, p0 + p] C[mu, q0 + q], C (nao x nmo) row-major
__global__ void k_stda_charges(int natm, const int* __restrict__ off, int nmo, const double* __restrict__ c,
                               int p0, int np, int q0, int nq, double* __restrict__ out) {
  const long total = (long)np * nq * natm;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int a = (int)(t % natm);
    const long pq = t / natm;
    const int p = (int)(pq / nq), q = (int)(pq % nq);
    double s = 0.0;
    for (int mu = off[a]; mu < off[a + 1]; ++mu) s += c[(long)mu * nmo + p0 + p] * c[(long)mu * nmo + q0 + q];
    out[t] = s;
  }
}

int bad(const char* what, const char* msg) { return set_error(XT_ERR_ARG, (std::string(what) + ": " + msg).c_str()); }

// host-only descriptor checks
int check_desc(const char* what, const xt_stda_desc* desc) {
  if (!desc) return bad(what, "null descriptor");
  const xt_stda_desc& d = *desc;
  if (d.natm < 0) return bad(what, "natm < 0");
  if (d.nocc_a < 0 || d.nvir_a < 0 || d.nocc_b < 0 || d.nvir_b < 0 || d.nc < 0 || d.no < 0 || d.nv < 0)
    return bad(what, "negative orbital count");
  if (d.spin_adapted != 0 && d.spin_adapted != 1) return bad(what, "spin_adapted must be 0 or 1");
  if (d.correct != 0 && d.correct != 1) return bad(what, "correct must be 0 or 1");
  if (d.spin_adapted && (d.nocc_a != d.nc + d.no || d.nvir_a != d.nv || d.nocc_b != d.nc || d.nvir_b != d.no + d.nv))
    return bad(what, "inconsistent ROKS counts (need nocc_a = nc + no, nvir_a = nv, nocc_b = nc, nvir_b = no + nv)");
  if (d.spin_adapted && d.no > 0 && !(d.si > 0.0)) return bad(what, "spin adaptation with open shells needs si > 0");
  if (d.correct && !(d.sigma_k > 0.0)) return bad(what, "correct needs sigma_k > 0");
  return 0;
}

int check_list(const char* what, const xt_stda_desc& d, int n, const int* csf, const char* name) {
  if (n < 0) return bad(what, (std::string("negative length of ") + name).c_str());
  if (n > 0 && !csf) return bad(what, (std::string("null CSF list ") + name).c_str());
  for (long k = 0; k < n; ++k) {
    const int s = csf[3 * k], i = csf[3 * k + 1], a = csf[3 * k + 2];
    if (s != 0 && s != 1) return bad(what, (std::string(name) + ": spin must be 0 or 1 (entry " + std::to_string(k) + ")").c_str());
    const int no_s = s ? d.nocc_b : d.nocc_a, nv_s = s ? d.nvir_b : d.nvir_a;
    if (i < 0 || i >= no_s || a < 0 || a >= nv_s)
      return bad(what, (std::string(name) + ": index outside its block (entry " + std::to_string(k) + ")").c_str());
  }
  return 0;
}

// which spins the lists touch -> which operand pointers must be there
int check_ops(const char* what, const xt_stda_desc& d, const xt_stda_ops* ops, bool full, int n1, const int* l1, int n2,
              const int* l2) {
  if (!ops) return bad(what, "null operand table");
  bool used[2] = {false, false};
  for (long k = 0; k < n1; ++k) used[l1[3 * k]] = true;
  for (long k = 0; k < n2; ++k) used[l2[3 * k]] = true;
  const double* const* need[2][8] = {
      {&ops->q_ov_a, &ops->k_ov_a, &ops->q_oo_a, &ops->j_vv_a, &ops->f_oo_a, &ops->f_vv_a, &ops->h_oo_a, &ops->h_vv_a},
      {&ops->q_ov_b, &ops->k_ov_b, &ops->q_oo_b, &ops->j_vv_b, &ops->f_oo_b, &ops->f_vv_b, &ops->h_oo_b, &ops->h_vv_b}};
  // the X term couples CV(aa) and CV(bb) through the ROHF-type blocks of both spins
  const bool xterm = full && d.spin_adapted && d.no > 0 && (used[0] || used[1]);
  for (int s = 0; s < 2; ++s) {
    if (used[s]) {
      for (int k = 0; k < (full ? 6 : 4); ++k)
        if (!*need[s][k]) return bad(what, "null operand for a spin the list uses");
    }
    if (xterm && (!*need[s][6] || !*need[s][7])) return bad(what, "null ROHF-type Fock block (spin_adapted)");
  }
  return 0;
}

Gen make_gen(const xt_stda_desc& d, const xt_stda_ops& o) {
  Gen g;
  g.natm = d.natm;
  g.nocc[0] = d.nocc_a; g.nocc[1] = d.nocc_b; g.nvir[0] = d.nvir_a; g.nvir[1] = d.nvir_b;
  g.nc = d.nc; g.no = d.no; g.nv = d.nv;
  g.sa = d.spin_adapted && d.no > 0;
  g.c1 = g.c2 = g.c3 = 0.0;
  if (g.sa) {
    const double s = d.si, rt = sqrt((s + 1.0) / s);
    g.c1 = 0.5 * (1.0 - rt + 1.0 / (2.0 * s));
    g.c2 = 0.5 * (-1.0 + rt + 1.0 / (2.0 * s));
    g.c3 = 1.0 / (4.0 * s);
  }
  g.correct = d.correct; g.dmax = d.delta_max; g.sigk = d.correct ? d.sigma_k : 1.0;
  g.qov[0] = o.q_ov_a; g.qov[1] = o.q_ov_b; g.kov[0] = o.k_ov_a; g.kov[1] = o.k_ov_b;
  g.qoo[0] = o.q_oo_a; g.qoo[1] = o.q_oo_b; g.jvv[0] = o.j_vv_a; g.jvv[1] = o.j_vv_b;
  g.foo[0] = o.f_oo_a; g.foo[1] = o.f_oo_b; g.fvv[0] = o.f_vv_a; g.fvv[1] = o.f_vv_b;
  g.hoo[0] = o.h_oo_a; g.hoo[1] = o.h_oo_b; g.hvv[0] = o.h_vv_a; g.hvv[1] = o.h_vv_b;
  return g;
}

// a host list of count ints, copied into b
int upload_ints(const char* what, TmpMem<int>& b, const int* src, long count, hipStream_t st) {
  return upload(b, src, (size_t)count, XT_PTR_HOST, st, what);
}

}  // namespace

extern "C" int xt_stda_charges(const xt_stda_desc* desc, int spin, int nao, const int* ao_off, const double* cprime,
                               double* q_oo, double* q_ov, double* q_vv, void* stream) {
  const char* what = "xt_stda_charges";
  RET(check_desc(what, desc));
  const xt_stda_desc d = *desc;
  if (spin != 0 && spin != 1) return bad(what, "spin must be 0 or 1");
  if (nao < 0) return bad(what, "nao < 0");
  const int nocc = spin ? d.nocc_b : d.nocc_a, nvir = spin ? d.nvir_b : d.nvir_a, nmo = nocc + nvir;
  if (d.natm == 0 || nmo == 0) return 0;   // no work
  if (!ao_off) return bad(what, "null atom AO offsets");
  if (ao_off[0] < 0 || ao_off[d.natm] > nao) return bad(what, "atom AO offsets outside [0, nao]");
  for (int a = 0; a < d.natm; ++a)
    if (ao_off[a + 1] < ao_off[a]) return bad(what, "atom AO offsets must not decrease");
  if (!cprime && ao_off[d.natm] > ao_off[0]) return bad(what, "null coefficient matrix");
  if ((nocc > 0 && !q_oo) || (nocc > 0 && nvir > 0 && !q_ov) || (nvir > 0 && !q_vv)) return bad(what, "null output block");

  hipStream_t st = (hipStream_t)stream;
  TmpMem<int> off;
  RET(upload_ints(what, off, ao_off, d.natm + 1, st));
  auto launch = [&](int p0, int np, int q0, int nq, double* out) {
    const long total = (long)np * nq * d.natm;
    if (total <= 0) return;
    long nb = (total + 255) / 256;
    if (nb > 65536) nb = 65536;
    hipLaunchKernelGGL(k_stda_charges, dim3((unsigned)nb), dim3(256), 0, st, d.natm, off.p, nmo, cprime, p0,
                       np, q0, nq, out);
  };
  launch(0, nocc, 0, nocc, q_oo);
  launch(0, nocc, nocc, nvir, q_ov);
  launch(nocc, nvir, nocc, nvir, q_vv);
  HIPCHK(what, hipGetLastError());
  HIPCHK(what, hipStreamSynchronize(st));   // the offsets are released on return
  return 0;
}

extern "C" int xt_stda_half(const xt_stda_desc* desc, int spin, const double* gamma_k, const double* gamma_j,
                            const double* q_ov, const double* q_vv, double* k_ov, double* j_vv, void* stream) {
  const char* what = "xt_stda_half";
  RET(check_desc(what, desc));
  const xt_stda_desc d = *desc;
  if (spin != 0 && spin != 1) return bad(what, "spin must be 0 or 1");
  const int nocc = spin ? d.nocc_b : d.nocc_a, nvir = spin ? d.nvir_b : d.nvir_a;
  const long nov = (long)nocc * nvir, nvv = (long)nvir * nvir;
  if (d.natm == 0 || (nov == 0 && nvv == 0)) return 0;   // no work
  if ((nov > 0 && (!gamma_k || !q_ov || !k_ov)) || (nvv > 0 && (!gamma_j || !q_vv || !j_vv))) return bad(what, "null argument");
  // (pairs x natm) times the symmetric (natm x natm) gamma, in row chunks within the engine's row range
  auto product = [&](long rows, const double* q, const double* gam, double* out) -> int {
    const long chunk = 1L << 18;
    for (long r0 = 0; r0 < rows; r0 += chunk) {
      const int m = (int)(rows - r0 < chunk ? rows - r0 : chunk);
      RET(xt_dgemm(0, 0, m, d.natm, d.natm, 1.0, q + r0 * d.natm, d.natm, gam, d.natm, 0.0, out + r0 * d.natm, d.natm, stream));
    }
    return 0;
  };
  RET(product(nov, q_ov, gamma_k, k_ov));
  RET(product(nvv, q_vv, gamma_j, j_vv));
  return 0;
}

extern "C" int xt_stda_diag(const xt_stda_desc* desc, const xt_stda_ops* ops, int n, const int* csf, double* e,
                            double* kpp, void* stream) {
  const char* what = "xt_stda_diag";
  RET(check_desc(what, desc));
  const xt_stda_desc d = *desc;
  RET(check_list(what, d, n, csf, "csf"));
  if (n == 0) return 0;
  RET(check_ops(what, d, ops, true, n, csf, 0, nullptr));
  if (!e) return bad(what, "null output");
  hipStream_t st = (hipStream_t)stream;
  TmpMem<int> l;
  RET(upload_ints(what, l, csf, 3L * n, st));
  const int nt = (n + 15) / 16;
  hipLaunchKernelGGL(k_stda_diag, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, st, make_gen(d, *ops), l.p, n,
                     nt, e, kpp);
  HIPCHK(what, hipGetLastError());
  HIPCHK(what, hipStreamSynchronize(st));   // the list is released on return
  return 0;
}

extern "C" int xt_stda_select(const xt_stda_desc* desc, const xt_stda_ops* ops, int n_p, const int* csf_p,
                              const double* e_p, int n_n, const int* csf_n, const double* e_n, double* w, void* stream) {
  const char* what = "xt_stda_select";
  RET(check_desc(what, desc));
  const xt_stda_desc d = *desc;
  RET(check_list(what, d, n_p, csf_p, "csf_p"));
  RET(check_list(what, d, n_n, csf_n, "csf_n"));
  if (n_n == 0) return 0;
  if (!w || !e_n || (n_p > 0 && !e_p)) return bad(what, "null argument");
  RET(check_ops(what, d, ops, false, n_p, csf_p, n_n, csf_n));
  hipStream_t st = (hipStream_t)stream;
  TmpMem<int> lp, ln;
  if (n_p > 0) RET(upload_ints(what, lp, csf_p, 3L * n_p, st));
  RET(upload_ints(what, ln, csf_n, 3L * n_n, st));
  const int nt = (n_n + 15) / 16;
  hipLaunchKernelGGL(k_stda_select, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, st, make_gen(d, *ops), lp.p,
                     n_p, e_p, ln.p, n_n, e_n, nt, w);
  HIPCHK(what, hipGetLastError());
  HIPCHK(what, hipStreamSynchronize(st));   // the lists are released on return
  return 0;
}

extern "C" int xt_stda_matrix(const xt_stda_desc* desc, const xt_stda_ops* ops, int n, const int* csf, double* a,
                              void* stream) {
  const char* what = "xt_stda_matrix";
  RET(check_desc(what, desc));
  const xt_stda_desc d = *desc;
  RET(check_list(what, d, n, csf, "csf"));
  if (n == 0) return 0;
  if (!a) return bad(what, "null output");
  RET(check_ops(what, d, ops, true, n, csf, 0, nullptr));
  const int nt = (n + 15) / 16;
  const long nblk = ((long)nt * nt + 3) / 4;
  if (nblk > 0x7fffffffL) return bad(what, "list too long for one launch");
  hipStream_t st = (hipStream_t)stream;
  TmpMem<int> l;
  RET(upload_ints(what, l, csf, 3L * n, st));
  hipLaunchKernelGGL(k_stda_matrix, dim3((unsigned)nblk), dim3(256), 0, st, make_gen(d, *ops), l.p, n, nt, a);
  HIPCHK(what, hipGetLastError());
  HIPCHK(what, hipStreamSynchronize(st));   // the list is released on return
  return 0;
}
