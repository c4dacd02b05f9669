// xt_ctx: device-resident TDA operator and its C ABI (include/xtddft_amd.h).
//
// The reference forms AO transition densities, calls PySCF get_jk and
// nr_uks_fxc on them and projects back (XTDA.py:615-690).  Here the same
// operator is evaluated in the MO basis, with every tensor transformed once
// at setup and kept resident in HBM:
//
//   Bmo[P,p,q] = (C^T B_P C)_pq       DF factor in the MO basis
//   Phi[c,g,p] = (ao_c(g) C)_p        MO values / gradients on the grid
//
// and per xt_apply (nz trial vectors, one spin channel Ze = (nz, O, V)):
//   J   gamma[x,P] = sum_ch <Bmo[P,occ,vir], Ze_ch[x]>;  sigma += gamma . Bmo[:,occ,vir]
//   K   sigma[x] -= c_K sum_P Bmo[P,occ,occ] Ze[x] Bmo[P,vir,vir]          (sandwich)
//   XC  U_c = PhiV^c Ze^T ; rho1/wv/S on the grid (k_xc_*) ; sigma += S_c^T PhiV^c
//   1e  Fock (and Delta-A) MO products, or the orbital-energy diagonal (UTDA)
// all as strided FP64-MFMA GEMMs (xt_gemm.hip).  Algebraically identical to
// the reference's AO route (the projections are linear), different summation
// order: parity is to FP64 round-off, see tests/test_gpu_parity.py.
// This file: the context, the one-electron terms and xt_apply; the rest as xt_ctx.h lists.
#include <hip/hip_runtime.h>
#include <math.h>
#include "xt_ctx.h"
#include "xt_kernels.h"

using namespace xt;

static thread_local std::string g_err;
int xt::set_error(int code, const char* msg) { g_err = msg; return code; }

static int dim_of(const xt_desc& d) {
  const int nc = d.nc, no = d.no, nv = d.nv;
  switch (d.kind) {
    case XT_KIND_XTDA: case XT_KIND_UTDA: return (nc + no) * nv + nc * (no + nv);
    case XT_KIND_SF_DOWN: return (nc + no) * (no + nv);
    case XT_KIND_SF_UP: return nc * nv;
    case XT_KIND_XSF: return (nc + no) * (no + nv) - (d.remove ? 1 : 0);
  }
  return 0;
}

int xt::to_device(xt_ctx* c, double* dst, const double* src, size_t count, int ptr_kind) {
  HIPCHK("", hipMemcpyAsync(dst, src, count * sizeof(double),
                            ptr_kind == XT_PTR_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->st));
  return 0;
}

int xt::to_device(xt_ctx* c, DevBuf& dst, const double* src, size_t count, int ptr_kind) {
  RET(dst.ensure(count));
  return to_device(c, dst.p, src, count, ptr_kind);
}

// live timing of a tagged launch class (xt_set_profile): an event pair around it
int xt::prof_begin(xt_ctx* c, int tag, double flops, double bytes, bool* on) {
  *on = tag > 0 && tag < 6 && ((c->prof_mask >> tag) & 1);
  if (!*on) return 0;
  if ((int)c->pev.size() < c->pev_used + 2) {
    hipEvent_t a, b;
    HIPCHK("", hipEventCreate(&a)); HIPCHK("", hipEventCreate(&b));
    c->pev.push_back(a); c->pev.push_back(b);
    c->pev_tag.push_back(0); c->pev_tag.push_back(0);
  }
  c->pev_tag[c->pev_used] = tag;
  HIPCHK("", hipEventRecord(c->pev[c->pev_used], c->st));
  c->prof_flops[tag] += flops;
  c->prof_bytes[tag] += bytes;
  return 0;
}

int xt::prof_end(xt_ctx* c, int tag, bool on) {
  if (!on) return 0;
  HIPCHK("", hipEventRecord(c->pev[c->pev_used + 1], c->st));
  c->pev_used += 2;
  c->prof_launches[tag] += 1;
  return 0;
}

int xt::gemm(xt_ctx* c, const GemmDesc& g) {
  bool prof = false;
  const double nr = g.R > 0 ? g.R : 1, nb = (double)(g.nb1 > 0 ? g.nb1 : 1) * (g.nb2 > 0 ? g.nb2 : 1);
  // compulsory bytes: A and B read once, C written once (read too when beta != 0)
  const double bytes = g.bytes > 0 ? g.bytes
                                   : 8.0 * nb * (nr * ((double)g.M * g.K + (double)g.K * g.N) +
                                                 (g.beta != 0.0 ? 2.0 : 1.0) * g.M * (double)g.N);
  RET(prof_begin(c, g.tag, g.flops > 0 ? g.flops : 2.0 * g.M * (double)g.N * g.K * nr * nb, bytes, &prof));
  RET(run_gemm(g, c->st, c->ws, (size_t)512 << 20, 0, "", "dgemm launch failed"));   // 512 MiB split-K workspace cap
  return prof_end(c, g.tag, prof);
}

extern "C" {

int xt_set_profile(xt_ctx* c, int mask) {
  if (!c) return fail(XT_ERR_ARG, "null ctx");
  c->prof_mask = mask;
  return 0;
}

// device ms, launches and algorithmic flops of GEMM class `tag` in the last
// xt_apply (one launch = one GEMM call including its split-K reduce)
int xt_profile_stats(const xt_ctx* c, int tag, double* out3) {
  if (!c || !out3 || tag < 1 || tag > 5) return fail(XT_ERR_ARG, "bad argument");
  out3[0] = c->prof_ms[tag]; out3[1] = c->prof_launches[tag]; out3[2] = c->prof_flops[tag];
  return 0;
}

// compulsory HBM bytes of GEMM class `tag` in the last xt_apply (every operand
// read once, the output written once): the denominator of a traffic ratio
int xt_profile_bytes(const xt_ctx* c, int tag, double* bytes) {
  if (!c || !bytes || tag < 1 || tag > 5) return fail(XT_ERR_ARG, "bad argument");
  *bytes = c->prof_bytes[tag];
  return 0;
}

int xt_abi_version(void) { return XT_ABI_VERSION; }
const char* xt_last_error(void) { return g_err.c_str(); }

int xt_create(const xt_desc* desc, xt_ctx** out) {
  if (!desc || !out) return fail(XT_ERR_ARG, "null argument");
  const xt_desc& d = *desc;
  if (d.nao <= 0 || d.nmo <= 0 || d.nc < 0 || d.no < 0 || d.nv <= 0 || d.nc + d.no + d.nv != d.nmo)
    return fail(XT_ERR_ARG, "inconsistent orbital dimensions (need nc+no+nv == nmo)");
  if (d.kind < XT_KIND_XTDA || d.kind > XT_KIND_XSF) return fail(XT_ERR_ARG, "unknown kind");
  if (d.kind == XT_KIND_XTDA && !d.restricted) return fail(XT_ERR_ARG, "XTDA needs a ROKS reference");
  if (d.kind == XT_KIND_UTDA && d.restricted) return fail(XT_ERR_ARG, "UTDA needs a UKS reference");
  if (d.kind == XT_KIND_XTDA && d.si <= 0) return fail(XT_ERR_ARG, "XTDA needs spin > 0");
  if (d.kind == XT_KIND_XSF && d.sa > 0 && (d.no < 2 || !d.restricted))
    return fail(XT_ERR_ARG, "XSF spin adaptation needs ROKS with no >= 2 (2S-1 > 0)");
  if (d.kind == XT_KIND_XSF && d.remove && d.no < 1)
    return fail(XT_ERR_ARG, "XSF OO compression needs an open shell");
  if (d.xctype < XT_XC_NONE || d.xctype > XT_XC_MGGA) return fail(XT_ERR_ARG, "bad xctype");
  const bool sf = is_sf(d);
  if (sf && d.sf_kernel != XT_SF_ALDA0 && d.sf_kernel != XT_SF_MC) return fail(XT_ERR_ARG, "bad sf_kernel");
  // spin flip: ALDA0 uses densities only, the grid needs ao[0] only (SF_TDA.py:73-80); the
  // multicollinear kernel is GGA / MGGA-shaped over (s, grad s[, tau_s]) (SF_TDA.py:997-1041)
  const bool dens_only = sf && d.sf_kernel == XT_SF_ALDA0;
  HIPCHK("", hipSetDevice(d.device));
  xt_ctx* c = new xt_ctx();
  c->d = d;
  c->nbasis = d.restricted ? 1 : 2;
  c->ncomp = ((d.xctype == XT_XC_GGA || d.xctype == XT_XC_MGGA) && !dens_only) ? 4 : 1;
  c->nkc = (d.xctype == XT_XC_MGGA && !dens_only) ? 5 : c->ncomp;
  const int nb = d.restricted ? 0 : 1;   // beta basis index
  if (d.kind == XT_KIND_XTDA || d.kind == XT_KIND_UTDA) {
    c->nchan = 2; c->O = d.nc + d.no; c->V = d.no + d.nv; c->v0 = d.nc;
    c->occ_basis[0] = 0; c->vir_basis[0] = 0; c->occ_basis[1] = nb; c->vir_basis[1] = nb;
  } else if (d.kind == XT_KIND_SF_UP) {
    c->nchan = 1; c->O = d.nc; c->V = d.nv; c->v0 = d.nc + d.no;
    c->occ_basis[0] = nb; c->vir_basis[0] = 0;
  } else {
    c->nchan = 1; c->O = d.nc + d.no; c->V = d.no + d.nv; c->v0 = d.nc;
    c->occ_basis[0] = 0; c->vir_basis[0] = nb;
  }
  // exchange coefficients (XTDA.py:522-539 ; SF_TDA.py:273-277)
  const bool hf = (d.xctype == XT_XC_NONE);
  const double hyb = hf ? 1.0 : d.hyb;
  c->ck = hyb; c->ck_lr = 0.0;
  if (!hf && d.omega != 0.0) {
    if (sf) c->ck_lr = d.alpha - d.hyb;
    else if (d.alpha == 0.0) c->ck_lr = -d.hyb;
    else if (d.hyb == 0.0) { c->ck = 0.0; c->ck_lr = d.alpha; }
    else c->ck_lr = d.alpha - d.hyb;
  }
  for (int i = 0; i < 5; ++i) (void)hipEventCreate(&c->ev[i]);
  {
    // the only environment knobs, read here once per context (test hooks): which XC kernels
    // run the fused classes outside their automatic ranges (tests/test_gpu_variants.py), and
    // XT_CHUNK_BYTES below.
    // Defaults: dedicated M-backward for O <= 128, rho-forward for O > 64 and the
    // small-O rho-forward for O <= 48 (from 8 trial pairs), the engine's fused modes
    // otherwise (where they win or the dedicated kernels do not fit).  XT_W_KERNEL: 0 the
    // engine, 1 the O > 64 kernel, 3 the small-O kernel wherever they fit
    const char* em = getenv("XT_M_KERNEL");
    c->m_kernel = !(em && atoi(em) == 0);
    const char* ew = getenv("XT_W_KERNEL");
    c->w_kernel = ew ? (atoi(ew) == 0 ? 0 : atoi(ew) == 3 ? 3 : 1) : 2;
    // XT_CHUNK_BYTES (tests/test_gpu_chunks.py): caps the byte budgets of the chunked loops
    // over grid points and aux rows (xt_set_grid, df_to_mo, sandwich, exchange_main,
    // xc_response) so that small problems run several chunks and a ragged last one.  Unset
    // or <= 0: every budget is its default; the floors (one aux row, one grid row, 64 XC
    // points) hold either way
    const char* ec = getenv("XT_CHUNK_BYTES");
    const long long cb = ec ? atoll(ec) : 0;
    c->chunk_bytes = cb > 0 ? (size_t)cb : 0;
  }
  *out = c;
  return 0;
}

int xt_destroy(xt_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->d.device);
  DevBuf* bufs[] = {&c->C, &c->Bmo, &c->Bmo_lr, &c->Phi, &c->kern, &c->F, &c->eps, &c->vects,
                    &c->ze, &c->acc, &c->kx, &c->zr, &c->tbuf, &c->ubuf, &c->gam, &c->gam2, &c->ws,
                    &c->stage, &c->stage2, &c->zin, &c->sout, &c->trace, &c->zp, &c->accT, &c->wbuf, &c->taubuf,
                    &c->Kx, &c->nlcPhi, &c->nlcG, &c->nlcU, &c->nlcR};
  for (DevBuf* b : bufs) b->release();
  for (int i = 0; i < 5; ++i) (void)hipEventDestroy(c->ev[i]);
  for (hipEvent_t e : c->pev) (void)hipEventDestroy(e);
  delete c;
  return 0;
}

int xt_set_stream(xt_ctx* c, void* s) {
  if (!c) return fail(XT_ERR_ARG, "null ctx");
  c->st = (hipStream_t)s;
  return 0;
}

int xt_dim(const xt_ctx* c) { return c ? dim_of(c->d) : 0; }

int xt_last_timings(const xt_ctx* c, double* out4) {
  if (!c || !out4) return fail(XT_ERR_ARG, "null argument");
  for (int i = 0; i < 4; ++i) out4[i] = c->timings[i];
  return 0;
}

int xt_set_orbitals(xt_ctx* c, const double* ca, const double* cb, int ptr_kind) {
  if (!c || !ca) return fail(XT_ERR_ARG, "null argument");
  (void)hipSetDevice(c->d.device);
  const size_t nn = (size_t)c->d.nao * c->d.nmo;
  RET(c->C.ensure(nn * c->nbasis));
  RET(to_device(c, c->C.p, ca, nn, ptr_kind));
  if (c->nbasis == 2) {
    if (!cb) return fail(XT_ERR_ARG, "UKS needs beta orbitals");
    RET(to_device(c, c->C.p + nn, cb, nn, ptr_kind));
  }
  c->has_orb = true;
  c->kx_valid = false;
  c->has_nlc = false;   // its MO values belong to the previous orbitals
  return 0;
}

int xt_set_fock_mo(xt_ctx* c, const double* fa, const double* fb, const double* fa_hf,
                   const double* fb_hf, int ptr_kind) {
  if (!c || !fa || !fb) return fail(XT_ERR_ARG, "null argument");
  (void)hipSetDevice(c->d.device);
  const size_t mm = (size_t)c->d.nmo * c->d.nmo;
  // F layout: [fa, fb, fa_hf, fb_hf, fs = (fb_hf - fa_hf)/2, dF = fb_hf - fa_hf]
  RET(c->F.ensure(6 * mm));
  const double* srcs[4] = {fa, fb, fa_hf ? fa_hf : fa, fb_hf ? fb_hf : fb};
  for (int i = 0; i < 4; ++i) RET(to_device(c, c->F.p + i * mm, srcs[i], mm, ptr_kind));
  // fs and dF via a tiny GEMM-free host round trip is avoided: use geam-like GEMM with identity?
  // simpler: stage on host (nmo^2 is small)
  std::vector<double> a(mm), b(mm), s(mm), df(mm);
  HIPCHK("", hipMemcpyAsync(a.data(), c->F.p + 2 * mm, mm * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK("", hipMemcpyAsync(b.data(), c->F.p + 3 * mm, mm * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK("", hipStreamSynchronize(c->st));
  for (size_t i = 0; i < mm; ++i) { df[i] = b[i] - a[i]; s[i] = 0.5 * df[i]; }
  HIPCHK("", hipMemcpy(c->F.p + 4 * mm, s.data(), mm * 8, hipMemcpyHostToDevice));
  HIPCHK("", hipMemcpy(c->F.p + 5 * mm, df.data(), mm * 8, hipMemcpyHostToDevice));
  c->has_fock = true;
  return 0;
}

int xt_set_orbital_energies(xt_ctx* c, const double* ea, const double* eb, int ptr_kind) {
  if (!c || !ea || !eb) return fail(XT_ERR_ARG, "null argument");
  (void)hipSetDevice(c->d.device);
  const size_t n = c->d.nmo;
  RET(c->eps.ensure(2 * n));
  RET(to_device(c, c->eps.p, ea, n, ptr_kind));
  RET(to_device(c, c->eps.p + n, eb, n, ptr_kind));
  c->has_eps = true;
  return 0;
}

int xt_set_oo_basis(xt_ctx* c, const double* vects, int ptr_kind) {
  if (!c || (!vects && c->d.no > 1)) return fail(XT_ERR_ARG, "null argument");
  (void)hipSetDevice(c->d.device);
  const size_t n = (size_t)c->d.no * c->d.no * (c->d.no * c->d.no - 1);
  if (n > 0) RET(to_device(c, c->vects, vects, n, ptr_kind));
  c->has_vects = true;
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// building blocks
// ---------------------------------------------------------------------------
// S[x] += alpha * Z[x] . F[fr0:, fc0:]   (Z: nr x K rows; F block K x ncl, row-major in nmo)
int xt::right_mo(xt_ctx* c, int nz, int nr, int K, int ncl, const double* Z, long ldZ, long svZ, const double* F,
                 long sFk, long sFn, double* S, long ldS, long svS, double alpha) {
  if (nr <= 0 || K <= 0 || ncl <= 0 || alpha == 0.0) return 0;
  GemmDesc g;
  g.M = nr; g.N = ncl; g.K = K; g.nb1 = nz;
  g.A = Z; g.sAm = ldZ; g.sAk = 1; g.sAb1 = svZ;
  g.B = F; g.sBk = sFk; g.sBn = sFn;
  g.C = S; g.ldc = ldS; g.sCb1 = svS;
  g.alpha = alpha; g.beta = 1.0;
  return gemm(c, g);
}

// S[x] += alpha * F . Z[x]   (F block nr x K with strides (sFm, sFk))
int xt::left_mo(xt_ctx* c, int nz, int nr, int K, int ncl, const double* F, long sFm, long sFk, const double* Z,
                long ldZ, long svZ, double* S, long ldS, long svS, double alpha) {
  if (nr <= 0 || K <= 0 || ncl <= 0 || alpha == 0.0) return 0;
  GemmDesc g;
  g.M = nr; g.N = ncl; g.K = K; g.nb1 = nz;
  g.A = F; g.sAm = sFm; g.sAk = sFk;
  g.B = Z; g.sBk = ldZ; g.sBn = 1; g.sBb1 = svZ;
  g.C = S; g.ldc = ldS; g.sCb1 = svS;
  g.alpha = alpha; g.beta = 1.0;
  return gemm(c, g);
}

// channel groups (xt_ctx.h)
int xt::channel_groups(const xt_ctx* c, Group* g) {
  if (c->nchan == 2 && c->occ_basis[0] == c->occ_basis[1] && c->vir_basis[0] == c->vir_basis[1]) {
    g[0] = {0, 2, c->occ_basis[0], c->vir_basis[0]};
    return 1;
  }
  for (int ch = 0; ch < c->nchan; ++ch) g[ch] = {ch, 1, c->occ_basis[ch], c->vir_basis[ch]};
  return c->nchan;
}

// ---------------------------------------------------------------------------
// the hot path
// ---------------------------------------------------------------------------
extern "C" int xt_apply(xt_ctx* c, int nz, const double* z, double* sigma, int ptr_kind) {
  if (!c || !z || !sigma) return fail(XT_ERR_ARG, "null argument");
  if (nz <= 0) return 0;
  const xt_desc& d = c->d;
  if (!c->has_orb) return fail(XT_ERR_STATE, "orbitals not set");
  if (!c->has_df && (d.naux > 0)) return fail(XT_ERR_STATE, "DF factor not set");
  if (d.omega != 0.0 && c->ck_lr != 0.0 && !c->has_lr && d.naux > 0)
    return fail(XT_ERR_STATE, "range-separated exchange needs the long-range DF factor");
  if (d.xctype != XT_XC_NONE && d.ngrid > 0 && !c->has_grid) return fail(XT_ERR_STATE, "grid not set");
  const bool xsf = d.kind == XT_KIND_XSF;
  if (d.add_local && d.kind != XT_KIND_UTDA && !c->has_fock) return fail(XT_ERR_STATE, "Fock matrices not set");
  if (d.add_local && d.kind == XT_KIND_UTDA && !c->has_eps) return fail(XT_ERR_STATE, "orbital energies not set");
  if (xsf && d.remove && !c->has_vects) return fail(XT_ERR_STATE, "OO basis not set");
  (void)hipSetDevice(d.device);
  const int O = c->O, V = c->V, nmo = d.nmo, nch = c->nchan;
  const long chs = (long)nz * O * V;
  const long mm = (long)nmo * nmo;
  const int dim = dim_of(d);

  const double* zd = z;
  double* sd = sigma;
  if (ptr_kind == XT_PTR_HOST) {
    RET(c->zin.ensure((size_t)nz * dim));
    RET(c->sout.ensure((size_t)nz * dim));
    HIPCHK("", hipMemcpyAsync(c->zin.p, z, (size_t)nz * dim * 8, hipMemcpyHostToDevice, c->st));
    zd = c->zin.p; sd = c->sout.p;
  }
  RET(c->ze.ensure(nch * chs));
  RET(c->acc.ensure(nch * chs));
  c->pev_used = 0;
  for (int t = 0; t < 6; ++t) { c->prof_flops[t] = 0.0; c->prof_bytes[t] = 0.0; c->prof_ms[t] = 0.0; c->prof_launches[t] = 0; }
  HIPCHK("", hipEventRecord(c->ev[0], c->st));
  // ---- embed trial vectors -------------------------------------------------
  if (d.kind == XT_KIND_XTDA || d.kind == XT_KIND_UTDA) embed_xtda(c->st, nz, d.nc, d.no, d.nv, zd, c->ze.p);
  else if (xsf) xsf_assemble(c->st, nz, d.nc, d.no, d.nv, d.remove, c->vects.p, zd, c->ze.p);
  else HIPCHK("", hipMemcpyAsync(c->ze.p, zd, chs * 8, hipMemcpyDeviceToDevice, c->st));
  HIPCHK("", hipMemsetAsync(c->acc.p, 0, nch * chs * 8, c->st));
  // Zp gets zeroed slack: the fused rho-forward kernels read whole a-tiles (up to 31
  // columns past the last channel's V, weighted by zero) and whole 8-row occupied
  // blocks (up to 7 rows of nch nz V past O, multiplied by zero PhiO rows)
  const long zslack = 8L * nch * nz * V + 64;
  RET(c->zp.ensure(nch * chs + zslack));
  HIPCHK("", hipMemsetAsync(c->zp.p + nch * chs, 0, zslack * 8, c->st));
  RET(c->accT.ensure(nch * chs));
  HIPCHK("", hipMemsetAsync(c->accT.p, 0, nch * chs * 8, c->st));
  Group grp[2];
  const int ngrp = channel_groups(c, grp);
  for (int q = 0; q < ngrp; ++q)   // Zp_g (O, nzg, V) = permuted Ze_g
    permute_xi(c->st, grp[q].nch * nz, O, V, c->ze.p + grp[q].ch0 * chs, c->zp.p + grp[q].ch0 * chs);

  // ---- one-electron terms (rank-local) --------------------------------------
  if (d.add_local) {
    if (d.kind == XT_KIND_UTDA) {
      ediag(c->st, nz, O, V, nmo, c->v0, c->eps.p, c->ze.p, c->acc.p);
    } else {
      for (int ch = 0; ch < nch; ++ch) {
        // channel Fock matrices: XTDA alpha/beta ; SF-down/XSF vir=FB occ=FA ; SF-up vir=FA occ=FB
        const double* Fv; const double* Fo;
        if (d.kind == XT_KIND_XTDA) { Fv = Fo = c->F.p + ch * mm; }
        else if (d.kind == XT_KIND_SF_UP) { Fv = c->F.p; Fo = c->F.p + mm; }
        else { Fv = c->F.p + mm; Fo = c->F.p; }
        RET(right_mo(c, nz, O, V, V, c->ze.p + ch * chs, V, (long)O * V, Fv + (long)c->v0 * nmo + c->v0,
                     nmo, 1, c->acc.p + ch * chs, V, (long)O * V, 1.0));
        RET(left_mo(c, nz, O, O, V, Fo, nmo, 1, c->ze.p + ch * chs, V, (long)O * V,
                    c->acc.p + ch * chs, V, (long)O * V, -1.0));
      }
      if (d.kind == XT_KIND_XTDA) {
        // spin-adaptation Delta-A on the CV blocks (XTDA.py:636-684)
        const double si = d.si;
        const double cp = 0.5 * (1 - sqrt((si + 1) / si) + 1 / (2 * si));
        const double cm = 0.5 * (-1 + sqrt((si + 1) / si) + 1 / (2 * si));
        const double cx = 0.5 / (2 * si);
        const int nc = d.nc, no = d.no, nv = d.nv;
        const double* dF = c->F.p + 5 * mm;           // fb_hf - fa_hf
        const double* dv = dF + (long)(nc + no) * nmo + (nc + no);
        const double* dov = dF;                       // core-core block
        const long sv = (long)O * V;
        for (int src = 0; src < 2; ++src) {
          const double* Zs = c->ze.p + src * chs + no;      // CV block of channel src
          for (int dst = 0; dst < 2; ++dst) {
            double* Sd = c->acc.p + dst * chs + no;
            double av, ao;
            if (src == dst) { av = (dst == 0) ? cp : cm; ao = (dst == 0) ? cm : cp; }
            else { av = -cx; ao = -cx; }
            RET(right_mo(c, nz, nc, nv, nv, Zs, V, sv, dv, nmo, 1, Sd, V, sv, av));
            RET(left_mo(c, nz, nc, nc, nv, dov, nmo, 1, Zs, V, sv, Sd, V, sv, ao));
          }
        }
      }
    }
  }
  HIPCHK("", hipEventRecord(c->ev[1], c->st));

  // ---- Coulomb / exchange ----------------------------------------------------
  if (d.naux > 0) RET(jk_response(c, nz));
  HIPCHK("", hipEventRecord(c->ev[2], c->st));

  // ---- XC ----------------------------------------------------------------------
  if (d.xctype != XT_XC_NONE && d.ngrid > 0) RET(xc_response(c, nz));
  if (c->has_nlc) RET(nlc_response(c, nz));
  for (int q = 0; q < ngrp; ++q)   // acc_g += accT_g (left-contraction results)
    permute_add(c->st, grp[q].nch * nz, O, V, 1.0, c->accT.p + grp[q].ch0 * chs, c->acc.p + grp[q].ch0 * chs);
  HIPCHK("", hipEventRecord(c->ev[3], c->st));

  // ---- extract -----------------------------------------------------------------
  if (d.kind == XT_KIND_XTDA || d.kind == XT_KIND_UTDA) extract_xtda(c->st, nz, d.nc, d.no, d.nv, c->acc.p, nullptr, sd);
  else if (xsf) xsf_extract(c->st, nz, d.nc, d.no, d.nv, d.remove, c->vects.p, c->acc.p, sd);
  else HIPCHK("", hipMemcpyAsync(sd, c->acc.p, chs * 8, hipMemcpyDeviceToDevice, c->st));
  HIPCHK("", hipEventRecord(c->ev[4], c->st));
  if (ptr_kind == XT_PTR_HOST)
    HIPCHK("", hipMemcpyAsync(sigma, c->sout.p, (size_t)nz * dim * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK("", hipEventSynchronize(c->ev[4]));
  float t01, t12, t23, t04;
  (void)hipEventElapsedTime(&t01, c->ev[0], c->ev[1]);
  (void)hipEventElapsedTime(&t12, c->ev[1], c->ev[2]);
  (void)hipEventElapsedTime(&t23, c->ev[2], c->ev[3]);
  (void)hipEventElapsedTime(&t04, c->ev[0], c->ev[4]);
  c->timings[0] = t12; c->timings[1] = t23; c->timings[2] = t01; c->timings[3] = t04;
  for (int i = 0; i < c->pev_used; i += 2) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->pev[i], c->pev[i + 1]);
    c->prof_ms[c->pev_tag[i]] += ms;
  }
  if (ptr_kind == XT_PTR_HOST) HIPCHK("", hipStreamSynchronize(c->st));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(XT_ERR_HIP, std::string("kernel error: ") + hipGetErrorString(e));
  return 0;
}
