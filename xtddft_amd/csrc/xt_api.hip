// xt_api: the entry points of include/xtddft_amd.h that take no operator context -- the
// GEMM engine (xt_dgemm*, xt_gemm_plan / xt_gemm_run), the Davidson helper kernels and the
// integral / AO evaluators.  Host code only: argument checks in front of the launchers.
#include <hip/hip_runtime.h>
#include <cmath>
#include <vector>
#include "xt_host.h"
#include "xt_kernels.h"

using namespace xt;

// ---------------------------------------------------------------------------
// device linear algebra for the Davidson solver
// ---------------------------------------------------------------------------
// ws_cap: split-K workspace cap in bytes (0: the default 256 MiB)
static int run_desc(const GemmDesc& g, void* stream, size_t ws_cap = 0) {
  // the engine's own layout and addressing rules, before the first HIP call
  if (g.M <= 0 || g.N <= 0) return 0;   // nothing to do (dgemm() launches nothing)
  if (dgemm_check(g)) return fail(XT_ERR_ARG, "dgemm: operand layout or stride not addressable");
  // split-K workspace per HIP device (the caller's current device owns the
  // stream and the operands)
  int dev = 0;
  HIPCHK("", hipGetDevice(&dev));
  static thread_local std::vector<DevBuf> ws_dev;
  if ((int)ws_dev.size() <= dev) ws_dev.resize(dev + 1);
  return run_gemm(g, (hipStream_t)stream, ws_dev[dev], ws_cap > 0 ? ws_cap : (size_t)256 << 20, ws_cap, "",
                  "dgemm launch failed");
}

extern "C" int xt_dgemm(int transa, int transb, int m, int n, int k, double alpha,
                        const double* a, long lda, const double* b, long ldb, double beta,
                        double* cc, long ldc, void* stream) {
  if (m < 0 || n < 0 || k < 0) return fail(XT_ERR_ARG, "xt_dgemm: negative size");
  // stored row lengths: A is (m x k) or, transposed, (k x m); B (k x n) or (n x k)
  if (lda < (transa ? m : k)) return fail(XT_ERR_ARG, "xt_dgemm: lda smaller than a stored row of A");
  if (ldb < (transb ? k : n)) return fail(XT_ERR_ARG, "xt_dgemm: ldb smaller than a stored row of B");
  if (ldc < n) return fail(XT_ERR_ARG, "xt_dgemm: ldc < n");
  if ((long)m * n > 0 && (!cc || (k > 0 && (!a || !b)))) return fail(XT_ERR_ARG, "xt_dgemm: null operand");
  GemmDesc g;
  g.M = m; g.N = n; g.K = k;
  g.A = a; if (transa) { g.sAm = 1; g.sAk = lda; } else { g.sAm = lda; g.sAk = 1; }
  g.B = b; if (transb) { g.sBk = 1; g.sBn = ldb; } else { g.sBk = ldb; g.sBn = 1; }
  g.C = cc; g.ldc = ldc; g.alpha = alpha; g.beta = beta;
  return run_desc(g, stream);
}

extern "C" int xt_dgemm_strided(int m, int n, int k, int r, int nbatch, double alpha,
                                const double* a, long sAm, long sAk, long sAr, long sAb,
                                const double* b, long sBk, long sBn, long sBr, long sBb, double beta,
                                double* cc, long ldc, long sCb, void* stream) {
  if (m < 0 || n < 0 || k < 0 || r < 1 || nbatch < 1) return fail(XT_ERR_ARG, "xt_dgemm_strided: bad sizes");
  if (sAm != 1 && sAk != 1) return fail(XT_ERR_ARG, "xt_dgemm_strided: A needs a unit m or k stride");
  if (sBn != 1 && sBk != 1) return fail(XT_ERR_ARG, "xt_dgemm_strided: B needs a unit k or n stride");
  if (sAm < 0 || sAk < 0 || sAr < 0 || sAb < 0 || sBk < 0 || sBn < 0 || sBr < 0 || sBb < 0 || sCb < 0)
    return fail(XT_ERR_ARG, "xt_dgemm_strided: negative stride");
  if (ldc < n) return fail(XT_ERR_ARG, "xt_dgemm_strided: ldc < n");
  if ((long)m * n > 0 && (!cc || (k > 0 && (!a || !b))))
    return fail(XT_ERR_ARG, "xt_dgemm_strided: null operand");
  GemmDesc g;
  g.M = m; g.N = n; g.K = k; g.R = r; g.nb1 = nbatch;
  g.A = a; g.sAm = sAm; g.sAk = sAk; g.sAr = sAr; g.sAb1 = sAb;
  g.B = b; g.sBk = sBk; g.sBn = sBn; g.sBr = sBr; g.sBb1 = sBb;
  g.C = cc; g.ldc = ldc; g.sCb1 = sCb; g.alpha = alpha; g.beta = beta;
  return run_desc(g, stream);
}

// xt_gemm_desc -> GemmDesc after the checks xt_gemm_plan and xt_gemm_run share (host only)
static int desc_to_gemm(const xt_gemm_desc* dp, GemmDesc* out) {
  if (!dp) return fail(XT_ERR_ARG, "xt_gemm: null descriptor");
  const xt_gemm_desc& d = *dp;
  if (d.m < 0 || d.n < 0 || d.k < 0 || d.r < 1 || d.nb1 < 1 || d.nb2 < 1)
    return fail(XT_ERR_ARG, "xt_gemm: bad sizes (m, n, k >= 0; r, nb1, nb2 >= 1)");
  if ((long)d.nb1 * d.nb2 > 65535) return fail(XT_ERR_ARG, "xt_gemm: more than 65535 batches");
  if (d.sAm != 1 && d.sAk != 1) return fail(XT_ERR_ARG, "xt_gemm: A needs a unit m or k stride");
  if (d.sBn != 1 && d.sBk != 1) return fail(XT_ERR_ARG, "xt_gemm: B needs a unit k or n stride");
  if (d.sAm < 0 || d.sAk < 0 || d.sAr < 0 || d.sAb1 < 0 || d.sAb2 < 0 || d.sBk < 0 || d.sBn < 0 || d.sBr < 0 ||
      d.sBb1 < 0 || d.sBb2 < 0 || d.sCb1 < 0 || d.sCb2 < 0 || d.sAm_hi < 0 || d.sC_hi < 0)
    return fail(XT_ERR_ARG, "xt_gemm: negative stride");
  if (d.ldc < d.n) return fail(XT_ERR_ARG, "xt_gemm: ldc < n");
  if (d.rdiv < 0 || (d.rdiv > 0 && (d.sAm != 1 || d.sAk == 1)))
    return fail(XT_ERR_ARG, "xt_gemm: two-level rows (rdiv > 0) need A m-contiguous");
  if (d.max_split < 0 || d.ws_bytes < 0) return fail(XT_ERR_ARG, "xt_gemm: negative max_split or ws_bytes");
  const bool akc = d.sAk == 1, bkc = d.sBk == 1;
  // a tagged call site has one operand layout (launch_cfg, xt_gemm.hip)
  const bool tag_ok = d.tag == 0 || ((d.tag == 1 || d.tag == 4) && akc && !bkc) || (d.tag == 2 && akc && bkc) ||
                      ((d.tag == 3 || d.tag == 5) && !akc && !bkc);
  if (d.tag < 0 || d.tag > 5 || !tag_ok)
    return fail(XT_ERR_ARG, "xt_gemm: tag must be 0..5 with its layout (1, 4: A k / B n; 2: k / k; 3, 5: m / n)");
  GemmDesc g;
  g.M = d.m; g.N = d.n; g.K = d.k; g.R = d.r; g.nb1 = d.nb1; g.nb2 = d.nb2;
  g.alpha = d.alpha; g.beta = d.beta;
  g.sAm = d.sAm; g.sAk = d.sAk; g.sAr = d.sAr; g.sAb1 = d.sAb1; g.sAb2 = d.sAb2;
  g.sBk = d.sBk; g.sBn = d.sBn; g.sBr = d.sBr; g.sBb1 = d.sBb1; g.sBb2 = d.sBb2;
  g.ldc = d.ldc; g.sCb1 = d.sCb1; g.sCb2 = d.sCb2;
  g.rdiv = d.rdiv; g.sAm_hi = d.sAm_hi; g.sC_hi = d.sC_hi;
  g.max_split = d.max_split; g.tag = d.tag;
  if (g.M > 0 && g.N > 0 && dgemm_check(g)) return fail(XT_ERR_ARG, "xt_gemm: stride not addressable by the engine");
  *out = g;
  return 0;
}

extern "C" int xt_gemm_plan(const xt_gemm_desc* d, int* cfg, int* bm, int* bn, int* bk, int* nsplit, int* masked) {
  if (!cfg || !bm || !bn || !bk || !nsplit || !masked) return fail(XT_ERR_ARG, "xt_gemm_plan: null output");
  GemmDesc g;
  RET(desc_to_gemm(d, &g));
  *cfg = -1; *bm = *bn = *bk = 0; *nsplit = 0; *masked = 0;
  if (g.M == 0 || g.N == 0) return 0;   // dgemm() launches nothing
  GemmParams p; int c;
  plan_gemm(g, &p, &c);
  gemm_cfg_tile(c, bm, bn, bk);
  *cfg = c;
  if (g.K == 0) { *nsplit = 1; return 0; }   // C = beta C, one pass
  // run_desc hands dgemm() min(need, cap) + 8 bytes, cut to a caller's cap
  const size_t cap = d->ws_bytes > 0 ? (size_t)d->ws_bytes : ((size_t)256 << 20) + 8;
  *nsplit = dgemm_fit_split(p, true, cap);
  *masked = (p.R > 1 && g.K % *bk != 0) ? 1 : 0;
  return 0;
}

extern "C" int xt_gemm_run(const xt_gemm_desc* d, const double* a, const double* b, double* cc, void* stream) {
  GemmDesc g;
  RET(desc_to_gemm(d, &g));
  if ((long)g.M * g.N > 0 && (!cc || (g.K > 0 && (!a || !b)))) return fail(XT_ERR_ARG, "xt_gemm_run: null operand");
  g.A = a; g.B = b; g.C = cc;
  return run_desc(g, stream, (size_t)d->ws_bytes);
}

extern "C" int xt_precond(int nrow, int dim, const double* diag, const double* e, double shift,
                          const double* r, double* out, void* stream) {
  if (nrow < 0 || dim < 0) return fail(XT_ERR_ARG, "xt_precond: negative size");
  if (nrow == 0 || dim == 0) return 0;   // nothing to do, nothing touched
  if (!diag || !e || !r || !out) return fail(XT_ERR_ARG, "xt_precond: null argument");
  precond((hipStream_t)stream, nrow, dim, diag, e, shift, r, out);
  return hipGetLastError() == hipSuccess ? 0 : fail(XT_ERR_HIP, "precond launch failed");
}
extern "C" int xt_row_norms2(int nrow, int dim, const double* x, double* out, void* stream) {
  if (nrow < 0 || dim < 0) return fail(XT_ERR_ARG, "xt_row_norms2: negative size");
  if (nrow == 0 || dim == 0) return 0;   // nothing to do, nothing touched
  if (!x || !out) return fail(XT_ERR_ARG, "xt_row_norms2: null argument");
  row_norms2((hipStream_t)stream, nrow, dim, x, out);
  return hipGetLastError() == hipSuccess ? 0 : fail(XT_ERR_HIP, "row_norms2 launch failed");
}
extern "C" int xt_row_scale(int nrow, int dim, double* x, const double* s, void* stream) {
  if (nrow < 0 || dim < 0) return fail(XT_ERR_ARG, "xt_row_scale: negative size");
  if (nrow == 0 || dim == 0) return 0;   // nothing to do, nothing touched
  if (!x || !s) return fail(XT_ERR_ARG, "xt_row_scale: null argument");
  row_scale((hipStream_t)stream, nrow, dim, x, s);
  return hipGetLastError() == hipSuccess ? 0 : fail(XT_ERR_HIP, "row_scale launch failed");
}

extern "C" int xt_int3c2e_cart(int npair, const int* pair_info, const double* pair_prim, const double* eab,
                               int naux_shells, const int* aux_info, const double* aux_prim, const double* ek,
                               int lmax_orb, int lmax_aux, double omega, double* out, long ldo,
                               void* stream) {
  return xt_int2e_cart(npair, pair_info, pair_prim, eab, naux_shells, aux_info, aux_prim, ek, lmax_orb, lmax_aux,
                       omega, nullptr, nullptr, 0.0, 0, out, ldo, stream);
}

extern "C" int xt_int2e_cart(int npair, const int* pair_info, const double* pair_prim, const double* eab,
                             int nket, const int* ket_info, const double* ket_prim, const double* ek,
                             int lmax_orb, int lket, double omega, const double* q_bra, const double* q_ket,
                             double q_thr, int diag, double* out, long ldo, void* stream) {
  if (npair < 0 || nket < 0 || ldo < 0) return fail(XT_ERR_ARG, "xt_int2e_cart: negative size");
  if (lmax_orb < 0 || lket < 0 || lmax_orb > kIntMaxLOrb || 2 * lmax_orb + lket > kIntMaxL)
    return fail(XT_ERR_ARG, "xt_int2e_cart: orbital shells up to f and 2 l_orb + l_ket <= 13");
  if (omega < 0.0) return fail(XT_ERR_ARG, "xt_int2e_cart: omega < 0");
  if ((q_bra == nullptr) != (q_ket == nullptr)) return fail(XT_ERR_ARG, "xt_int2e_cart: give both bounds or none");
  if (diag && nket != npair) return fail(XT_ERR_ARG, "xt_int2e_cart: diag needs the ket table = the bra table");
  const int r = int2e_cart(npair, pair_info, pair_prim, eab, nket, ket_info, ket_prim, ek, lmax_orb, lket, omega,
                           q_bra, q_ket, q_thr, diag, out, ldo, (hipStream_t)stream);
  return r ? fail(r, "int2e launch failed") : 0;
}

extern "C" int xt_hint_cart(int nbra, const int* bra_info, const double* bra_prim, const double* eb, int nket,
                            const int* ket_info, const double* ket_prim, const double* ek, int lbra, int lket,
                            int cross, long nrow_tot, double* out, long ldo, void* stream) {
  if (nbra < 0 || nket < 0 || ldo < 0) return fail(XT_ERR_ARG, "xt_hint_cart: negative size");
  if (lbra < 0 || lket < 0 || lbra > kHintMaxLBra || lbra + lket > kHintMaxL)
    return fail(XT_ERR_ARG, "xt_hint_cart: bra order <= 8 and total order <= 14");
  if (cross != 0 && cross != 1) return fail(XT_ERR_ARG, "xt_hint_cart: cross must be 0 or 1");
  if (cross && nrow_tot <= 0) return fail(XT_ERR_ARG, "xt_hint_cart: cross needs nrow_tot > 0");
  if ((long)nbra * nket > 0 && (!bra_info || !bra_prim || !eb || !ket_info || !ket_prim || !ek || !out))
    return fail(XT_ERR_ARG, "xt_hint_cart: null table or output");
  const int r = hint_cart(nbra, bra_info, bra_prim, eb, nket, ket_info, ket_prim, ek, lbra, lket, cross, nrow_tot,
                          out, ldo, (hipStream_t)stream);
  return r ? fail(r, "hint launch failed") : 0;
}

extern "C" int xt_grad_jk(int nbra, const int* bra_info, const double* bra_prim, const double* eb,
                          const int* bra_ao, int nket, const int* ket_info, const double* ket_prim,
                          const double* ek, const int* ket_ao, int lbra, int lket, int nterm, const double* wj,
                          const double* wk, const double* p, const double* q, long nao, int strip, int natm,
                          double* work, long nwork, double* out, void* stream) {
  if (nbra < 0 || nket < 0 || nao < 0 || natm < 0 || nwork < 0) return fail(XT_ERR_ARG, "xt_grad_jk: negative size");
  if (strip < 1) return fail(XT_ERR_ARG, "xt_grad_jk: strip must be at least 1");
  if (lbra < 0 || lket < 0 || lbra > kHintMaxLBra || lbra + lket > kHintMaxL)
    return fail(XT_ERR_ARG, "xt_grad_jk: bra order <= 8 and total order <= 14");
  if (nterm < 1 || nterm > kGradMaxTerms) return fail(XT_ERR_ARG, "xt_grad_jk: nterm must be 1..8");
  if (!wj || !wk) return fail(XT_ERR_ARG, "xt_grad_jk: null weights");
  if (nbra == 0 || nket == 0 || natm == 0) return 0;   // nothing to add
  if (!bra_info || !bra_prim || !eb || !bra_ao || !ket_info || !ket_prim || !ek || !ket_ao || !p || !q || !work ||
      !out)
    return fail(XT_ERR_ARG, "xt_grad_jk: null table, density, workspace or output");
  if (nwork < grad_jk_work(nbra, nket, strip)) return fail(XT_ERR_ARG, "xt_grad_jk: workspace too small");
  const int r = grad_jk(nbra, bra_info, bra_prim, eb, bra_ao, nket, ket_info, ket_prim, ek, ket_ao, lbra, lket, nterm,
                        wj, wk, p, q, nao, strip, natm, work, out, (hipStream_t)stream);
  return r ? fail(r, "grad_jk launch failed") : 0;
}

// xt_grad_jk2 (omega = 0: 1/r12) and xt_grad_jk2_lr (omega > 0: erf(omega r12) / r12): one set of checks,
// every message under the entry's own name
static int grad_jk2_entry(const char* what, int nbra, const int* bra_info, const double* bra_prim, const double* eb,
                          const int* bra_ao, int nket, const int* ket_info, const double* ket_prim,
                          const double* ek, const int* ket_ao, int lbra, int lket, int nj, const double* wj,
                          const double* pj, const double* qj, int nk, const double* wk, const double* pk,
                          const double* qk, long nao, int strip, int natm, double* work, long nwork, double* out,
                          void* stream, double omega) {
  const std::string pre = err_prefix(what);
  if (nbra < 0 || nket < 0 || nao < 0 || natm < 0 || nwork < 0) return fail(XT_ERR_ARG, pre + "negative size");
  if (strip < 1) return fail(XT_ERR_ARG, pre + "strip must be at least 1");
  if (lbra < 0 || lket < 0 || lbra > kHintMaxLBra || lbra + lket > kHintMaxL)
    return fail(XT_ERR_ARG, pre + "bra order <= 8 and total order <= 14");
  if (nj < 0 || nj > kGradMaxTerms) return fail(XT_ERR_ARG, pre + "nj must be 0..8");
  if (nk < 0 || nk > kGradMaxTerms) return fail(XT_ERR_ARG, pre + "nk must be 0..8");
  if (nj + nk < 1) return fail(XT_ERR_ARG, pre + "nj and nk are both zero");
  if (nj > 0 && !wj) return fail(XT_ERR_ARG, pre + "null wj with nj > 0");
  if (nk > 0 && !wk) return fail(XT_ERR_ARG, pre + "null wk with nk > 0");
  if (nbra == 0 || nket == 0 || natm == 0) return 0;   // nothing to add
  if (nj > 0 && (!pj || !qj)) return fail(XT_ERR_ARG, pre + "null pj or qj with nj > 0");
  if (nk > 0 && (!pk || !qk)) return fail(XT_ERR_ARG, pre + "null pk or qk with nk > 0");
  if (!bra_info || !bra_prim || !eb || !bra_ao || !ket_info || !ket_prim || !ek || !ket_ao || !work || !out)
    return fail(XT_ERR_ARG, pre + "null table, workspace or output");
  if (nwork < grad_jk_work(nbra, nket, strip)) return fail(XT_ERR_ARG, pre + "workspace too small");
  const int r = grad_jk2(nbra, bra_info, bra_prim, eb, bra_ao, nket, ket_info, ket_prim, ek, ket_ao, lbra, lket, nj, wj,
                         pj, qj, nk, wk, pk, qk, nao, strip, natm, work, out, (hipStream_t)stream, omega);
  return r ? fail(r, omega > 0.0 ? "grad_jk2_lr launch failed" : "grad_jk2 launch failed") : 0;
}

extern "C" int xt_grad_jk2(int nbra, const int* bra_info, const double* bra_prim, const double* eb,
                           const int* bra_ao, int nket, const int* ket_info, const double* ket_prim,
                           const double* ek, const int* ket_ao, int lbra, int lket, int nj, const double* wj,
                           const double* pj, const double* qj, int nk, const double* wk, const double* pk,
                           const double* qk, long nao, int strip, int natm, double* work, long nwork, double* out,
                           void* stream) {
  return grad_jk2_entry("xt_grad_jk2", nbra, bra_info, bra_prim, eb, bra_ao, nket, ket_info, ket_prim, ek, ket_ao, lbra,
                        lket, nj, wj, pj, qj, nk, wk, pk, qk, nao, strip, natm, work, nwork, out, stream, 0.0);
}

extern "C" int xt_grad_jk2_lr(int nbra, const int* bra_info, const double* bra_prim, const double* eb,
                              const int* bra_ao, int nket, const int* ket_info, const double* ket_prim,
                              const double* ek, const int* ket_ao, int lbra, int lket, int nj, const double* wj,
                              const double* pj, const double* qj, int nk, const double* wk, const double* pk,
                              const double* qk, long nao, int strip, int natm, double* work, long nwork, double* out,
                              void* stream, double omega) {
  // a caller who wants 1/r12 uses xt_grad_jk2: zero, negative, NaN and inf are all refused
  if (!(omega > 0.0) || !std::isfinite(omega))
    return fail(XT_ERR_ARG, "xt_grad_jk2_lr: omega must be finite and > 0");
  return grad_jk2_entry("xt_grad_jk2_lr", nbra, bra_info, bra_prim, eb, bra_ao, nket, ket_info, ket_prim, ek, ket_ao,
                        lbra, lket, nj, wj, pj, qj, nk, wk, pk, qk, nao, strip, natm, work, nwork, out, stream, omega);
}

extern "C" int xt_eval_ao(int ngrid, const double* coords, int nshell, const int* shell_info,
                          const double* shell_data, const double* sph, const double* ao_norm, int deriv,
                          double* out, long ldo, long comp_stride, void* stream) {
  if (ngrid < 0 || nshell < 0 || ldo < 0 || comp_stride < 0) return fail(XT_ERR_ARG, "xt_eval_ao: negative size");
  if (deriv != 0 && deriv != 1) return fail(XT_ERR_ARG, "xt_eval_ao: deriv must be 0 or 1");
  const int r = eval_ao(ngrid, coords, nshell, shell_info, shell_data, sph, ao_norm, deriv, out, ldo, comp_stride,
                        (hipStream_t)stream);
  return r ? fail(r, "eval_ao launch failed") : 0;
}
