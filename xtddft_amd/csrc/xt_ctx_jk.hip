// xt_ctx_jk: the Coulomb / exchange part of the operator context -- everything that knows
// the layout of the MO factor and of the stored exchange:
//   Bmo[b][P][p][q]  nbasis blocks of naux rows of nmo x nmo (C_b^T B_P C_b); after xt_prepare
//                    on a partitioned context only this rank's aux window of each block
//   Kx_g[(i,a)][(j,b)]  per channel group the context's occupied rows i, row stride kx_ld
#include <hip/hip_runtime.h>
#include <math.h>
#include "xt_ctx.h"
#include "xt_kernels.h"

using namespace xt;

// a factor setter after a trim starts over with the full aux count (both factors must be set again)
static void untrim(xt_ctx* c) {
  if (!c->trimmed) return;
  c->d.naux = c->naux_full;
  c->Bmo.release(); c->Bmo_lr.release();
  c->has_df = c->has_lr = false;
  c->trimmed = false;
}

// Bmo[b][P] = C_b^T B_P C_b, chunked over P so host inputs stream through HBM.
// AO factor rows (np x nao x nao) -> MO factor Bmo[b][P] = C_b^T B_P C_b for
// P < np, rows np..naux_rows of each basis block zeroed (dst holds
// nbasis x naux_rows x nmo x nmo).
static int df_to_mo(xt_ctx* c, const double* cderi, int np_total, DevBuf& dst, int naux_rows, int ptr_kind) {
  const int nao = c->d.nao, nmo = c->d.nmo;
  const size_t mm = (size_t)nmo * nmo, aa = (size_t)nao * nao;
  RET(dst.ensure(mm * (size_t)naux_rows * c->nbasis));
  if (naux_rows > np_total)
    for (int b = 0; b < c->nbasis; ++b)
      HIPCHK("", hipMemsetAsync(dst.p + ((size_t)b * naux_rows + np_total) * mm, 0,
                                (size_t)(naux_rows - np_total) * mm * 8, c->st));
  if (np_total <= 0) return 0;
  const size_t budget = chunk_budget(c, (size_t)2 << 30);   // bytes per staging buffer
  int pc = (int)(budget / (8 * (aa > mm ? aa : mm)));
  if (pc < 1) pc = 1;
  if (pc > np_total) pc = np_total;
  RET(c->stage2.ensure((size_t)pc * nao * nmo));
  if (ptr_kind == XT_PTR_HOST) RET(c->stage.ensure((size_t)pc * aa));
  for (int p0 = 0; p0 < np_total; p0 += pc) {
    const int np = (p0 + pc <= np_total) ? pc : np_total - p0;
    const double* src = cderi + (size_t)p0 * aa;
    if (ptr_kind == XT_PTR_HOST) {
      HIPCHK("", hipMemcpyAsync(c->stage.p, src, (size_t)np * aa * 8, hipMemcpyHostToDevice, c->st));
      src = c->stage.p;
    }
    for (int b = 0; b < c->nbasis; ++b) {
      const double* Cb = c->C.p + (size_t)b * nao * nmo;
      GemmDesc g1;   // T_P = B_P C  (nao x nmo)
      g1.M = nao; g1.N = nmo; g1.K = nao; g1.nb1 = np;
      g1.A = src; g1.sAm = nao; g1.sAk = 1; g1.sAb1 = (long)aa;
      g1.B = Cb; g1.sBk = nmo; g1.sBn = 1;
      g1.C = c->stage2.p; g1.ldc = nmo; g1.sCb1 = (long)nao * nmo;
      RET(gemm(c, g1));
      GemmDesc g2;   // Bmo_P = C^T T_P
      g2.M = nmo; g2.N = nmo; g2.K = nao; g2.nb1 = np;
      g2.A = Cb; g2.sAm = 1; g2.sAk = nmo;
      g2.B = c->stage2.p; g2.sBk = nmo; g2.sBn = 1; g2.sBb1 = (long)nao * nmo;
      g2.C = dst.p + ((size_t)b * naux_rows + p0) * mm; g2.ldc = nmo; g2.sCb1 = (long)mm;
      RET(gemm(c, g2));
    }
  }
  return 0;
}

extern "C" int xt_set_jk_df(xt_ctx* c, const double* cderi, int which, int ptr_kind) {
  if (!c || !cderi) return fail(XT_ERR_ARG, "null argument");
  if (which != 0 && which != 1) return fail(XT_ERR_ARG, "which must be 0 (full range) or 1 (long range)");
  if (!c->has_orb) return fail(XT_ERR_STATE, "xt_set_orbitals must precede xt_set_jk_df");
  (void)hipSetDevice(c->d.device);
  untrim(c);
  DevBuf& dst = which == 0 ? c->Bmo : c->Bmo_lr;
  RET(df_to_mo(c, cderi, c->d.naux, dst, c->d.naux, ptr_kind));
  HIPCHK("", hipStreamSynchronize(c->st));
  c->stage.release(); c->stage2.release();
  if (which == 0) c->has_df = true; else c->has_lr = true;
  c->kx_valid = false; c->k_resolved = -1;
  c->win_p0 = 0; c->win_np = -1;
  return 0;
}

// Re-lay an MO factor (nbasis blocks of old_rows x mm): each block keeps its rows
// [row0, row0 + keep) as the first of new_rows >= keep rows per block, the extra rows zero
// (grown for a common naux in xt_set_jk_eri8, trimmed to the aux window in trim_factor).
static int relay_factor(xt_ctx* c, DevBuf& B, int old_rows, int row0, int keep, int new_rows) {
  const size_t mm = (size_t)c->d.nmo * c->d.nmo;
  TmpBuf nb;
  RET(nb.ensure((size_t)c->nbasis * new_rows * mm));
  if (new_rows > keep) HIPCHK("", hipMemsetAsync(nb.p, 0, nb.n * 8, c->st));
  for (int b = 0; b < c->nbasis; ++b)
    if (keep > 0)
      HIPCHK("", hipMemcpyAsync(nb.p + (size_t)b * new_rows * mm, B.p + ((size_t)b * old_rows + row0) * mm,
                                (size_t)keep * mm * 8, hipMemcpyDeviceToDevice, c->st));
  HIPCHK("", hipStreamSynchronize(c->st));
  nb.swap(B);   // B takes the new rows, nb frees the old ones
  return 0;
}

extern "C" int xt_set_jk_eri8(xt_ctx* c, const double* eri, int which, double tol, int p_rank, int p_count,
                              int ptr_kind) {
  if (!c || !eri) return fail(XT_ERR_ARG, "null argument");
  if (which != 0 && which != 1) return fail(XT_ERR_ARG, "which must be 0 (full range) or 1 (long range)");
  if (p_count < 1 || p_rank < 0 || p_rank >= p_count) return fail(XT_ERR_ARG, "bad shard (p_rank, p_count)");
  if (!c->has_orb) return fail(XT_ERR_STATE, "xt_set_orbitals must precede xt_set_jk_eri8");
  (void)hipSetDevice(c->d.device);
  untrim(c);
  const int nao = c->d.nao;
  const long npair = (long)nao * (nao + 1) / 2;
  const size_t n8 = (size_t)npair * (npair + 1) / 2;
  const double* e = eri;
  TmpBuf ebuf, d, Lt, piv, Bao;
  RET(upload(ebuf, e, n8, ptr_kind, c->st, ""));
  RET(d.ensure(npair));
  RET(piv.ensure(2));
  eri_diag(c->st, npair, e, d.p);
  long cap = 8L * nao < npair ? 8L * nao : npair;
  RET(Lt.ensure((size_t)cap * npair));
  double thr = tol;
  int rank = 0;
  for (; rank < npair; ++rank) {
    argmax(c->st, npair, d.p, piv.p);
    double hv[2];
    HIPCHK("", hipMemcpyAsync(hv, piv.p, 16, hipMemcpyDeviceToHost, c->st));
    HIPCHK("", hipStreamSynchronize(c->st));
    if (rank == 0 && thr <= 0.0) thr = 1e-13 * hv[0];
    if (!(hv[0] > thr)) break;
    if (rank == cap) {   // grow the vector store
      const long ncap = 2 * cap < npair ? 2 * cap : npair;
      TmpBuf nl;
      RET(nl.ensure((size_t)ncap * npair));
      HIPCHK("", hipMemcpyAsync(nl.p, Lt.p, (size_t)cap * npair * 8, hipMemcpyDeviceToDevice, c->st));
      HIPCHK("", hipStreamSynchronize(c->st));
      nl.swap(Lt);
      cap = ncap;
    }
    chol_step(c->st, npair, rank, (long)hv[1], hv[0], e, Lt.p, npair, d.p);
  }
  ebuf.release(); d.release(); piv.release();
  // this rank's contiguous block of Cholesky vectors
  const int base = rank / p_count, rem = rank % p_count;
  const int lo = p_rank * base + (p_rank < rem ? p_rank : rem);
  const int np = base + (p_rank < rem ? 1 : 0);
  if (np > 0) {
    RET(Bao.ensure((size_t)np * nao * nao));
    chol_unpack(c->st, np, lo, nao, Lt.p, npair, Bao.p);
  }
  // common naux for the full-range and long-range factors (zero-padded)
  const bool other_set = which == 0 ? c->has_lr : c->has_df;
  int rows = np;
  if (other_set) {
    if (c->d.naux > rows) rows = c->d.naux;
    else if (c->d.naux < rows) RET(relay_factor(c, which == 0 ? c->Bmo_lr : c->Bmo, c->d.naux, 0, c->d.naux, rows));
  }
  DevBuf& dst = which == 0 ? c->Bmo : c->Bmo_lr;
  dst.release();
  RET(df_to_mo(c, Bao.p, np, dst, rows, XT_PTR_DEVICE));
  HIPCHK("", hipStreamSynchronize(c->st));
  Bao.release(); Lt.release(); c->stage.release(); c->stage2.release();
  c->d.naux = rows;
  c->chol_rank = rank;
  if (which == 0) c->has_df = true; else c->has_lr = true;
  c->kx_valid = false; c->k_resolved = -1;
  c->win_p0 = 0; c->win_np = -1;
  return 0;
}

extern "C" int xt_naux(const xt_ctx* c, int* naux_local, int* chol_rank) {
  if (!c) return fail(XT_ERR_ARG, "null argument");
  if (naux_local) *naux_local = c->d.naux;
  if (chol_rank) *chol_rank = c->chol_rank;
  return 0;
}

// S[x] += coef * sum_P Bo[P, ry0:+nry, rx0:+nrx] Z[x] Bv[P, cx0:+ncx, cy0:+ncy]
// Z[x] at Z + x*svZ with row stride ldZ; S[x] at S + x*svS, row stride ldS.
static int sandwich(xt_ctx* c, const double* Bo, const double* Bv, int nz,
                    int ry0, int nry, int rx0, int nrx, int cx0, int ncx, int cy0, int ncy,
                    const double* Z, long ldZ, long svZ, double* S, long ldS, long svS, double coef) {
  if (nry <= 0 || nrx <= 0 || ncx <= 0 || ncy <= 0 || coef == 0.0) return 0;
  const int naux = naux_w(c), nmo = c->d.nmo;
  if (naux <= 0) return 0;
  const long mm = (long)nmo * nmo;
  const double left = 2.0 * nry * nrx * (double)nz * ncx + 2.0 * nry * (double)nz * ncx * ncy;
  const double right = 2.0 * (double)nz * nrx * ncx * ncy + 2.0 * nry * nrx * (double)nz * ncy;
  const size_t budget = chunk_budget(c, (size_t)3 << 30);
  if (left <= right) {
    // T[P] (nry, nz, ncx) = Bo[P,rows] . Zr ; out(nry,nz,ncy) += T . Bv[P,cols]
    const size_t per = (size_t)nry * nz * ncx;
    int pc = (int)(budget / (8 * per)); if (pc < 1) pc = 1; if (pc > naux) pc = naux;
    RET(c->tbuf.ensure((size_t)pc * per));
    RET(c->zr.ensure((size_t)nrx * nz * ncx));
    RET(c->kx.ensure((size_t)nry * nz * ncy));
    // Zr[i][x][a] = Z[x][i][a]   (gather via GEMM-free copy: treat as batched strided copy)
    for (int x = 0; x < nz; ++x)
      HIPCHK("", hipMemcpy2DAsync(c->zr.p + (size_t)x * ncx, (size_t)nz * ncx * 8, Z + x * svZ, ldZ * 8,
                                  (size_t)ncx * 8, nrx, hipMemcpyDeviceToDevice, c->st));
    for (int p0 = 0; p0 < naux; p0 += pc) {
      const int np = (p0 + pc <= naux) ? pc : naux - p0;
      GemmDesc g1;
      g1.M = nry; g1.N = nz * ncx; g1.K = nrx; g1.nb1 = np;
      g1.A = Bo + p0 * mm + (long)ry0 * nmo + rx0; g1.sAm = nmo; g1.sAk = 1; g1.sAb1 = mm;
      g1.B = c->zr.p; g1.sBk = (long)nz * ncx; g1.sBn = 1;
      g1.C = c->tbuf.p; g1.ldc = (long)nz * ncx; g1.sCb1 = (long)per;
      RET(gemm(c, g1));
      GemmDesc g2;
      g2.M = nry * nz; g2.N = ncy; g2.K = ncx; g2.R = np;
      g2.A = c->tbuf.p; g2.sAm = ncx; g2.sAk = 1; g2.sAr = (long)per;
      g2.B = Bv + p0 * mm + (long)cx0 * nmo + cy0; g2.sBk = nmo; g2.sBn = 1; g2.sBr = mm;
      g2.C = c->kx.p; g2.ldc = ncy;
      g2.alpha = 1.0; g2.beta = (p0 == 0) ? 0.0 : 1.0;
      g2.tag = 1;
      RET(gemm(c, g2));
    }
    // S[x][j][b] += coef * kx[j][x][b]
    permute_add_strided(c->st, nz, nry, ncy, coef, c->kx.p, S, ldS, svS);
  } else {
    // W[P][x] (nrx, ncy) = Z[x] . Bv[P,cols] ; S[x] += coef * sum_P Bo[P,rows] W[P][x]
    const size_t per = (size_t)nz * nrx * ncy;
    int pc = (int)(budget / (8 * per)); if (pc < 1) pc = 1; if (pc > naux) pc = naux;
    RET(c->tbuf.ensure((size_t)pc * per));
    for (int p0 = 0; p0 < naux; p0 += pc) {
      const int np = (p0 + pc <= naux) ? pc : naux - p0;
      GemmDesc g1;
      g1.M = nrx; g1.N = ncy; g1.K = ncx; g1.nb1 = np; g1.nb2 = nz;
      g1.A = Z; g1.sAm = ldZ; g1.sAk = 1; g1.sAb1 = 0; g1.sAb2 = svZ;
      g1.B = Bv + p0 * mm + (long)cx0 * nmo + cy0; g1.sBk = nmo; g1.sBn = 1; g1.sBb1 = mm;
      g1.C = c->tbuf.p; g1.ldc = ncy; g1.sCb1 = (long)per; g1.sCb2 = (long)nrx * ncy;
      RET(gemm(c, g1));
      GemmDesc g2;
      g2.M = nry; g2.N = ncy; g2.K = nrx; g2.R = np; g2.nb1 = nz;
      g2.A = Bo + p0 * mm + (long)ry0 * nmo + rx0; g2.sAm = nmo; g2.sAk = 1; g2.sAr = mm;
      g2.B = c->tbuf.p; g2.sBk = ncy; g2.sBn = 1; g2.sBr = (long)per; g2.sBb1 = (long)nrx * ncy;
      g2.C = S; g2.ldc = ldS; g2.sCb1 = svS;
      g2.alpha = coef; g2.beta = 1.0;
      RET(gemm(c, g2));
    }
  }
  return 0;
}

// gamma[x,P] (+)= sum_{i,a} Z[x][i][a] Bmo[P][r0+i][c0+a]
static int coulomb_gamma(xt_ctx* c, const double* B, int nz, int r0, int nr, int c0, int ncl,
                         const double* Z, long ldZ, long svZ, double* gam, double beta) {
  const int nmo = c->d.nmo;
  GemmDesc g;
  g.M = nz; g.N = naux_w(c); g.K = ncl; g.R = nr;
  g.A = Z; g.sAm = svZ; g.sAk = 1; g.sAr = ldZ;
  g.B = B + (long)r0 * nmo + c0; g.sBn = (long)nmo * nmo; g.sBk = 1; g.sBr = nmo;
  g.C = gam; g.ldc = naux_w(c); g.beta = beta;
  return gemm(c, g);
}

// S[x][i][a] += coef * sum_P gamma[x,P] Bmo[P][r0+i][c0+a]
static int coulomb_project(xt_ctx* c, const double* B, int nz, int r0, int nr, int c0, int ncl,
                           const double* gam, double* S, long ldS, long svS, double coef) {
  const int nmo = c->d.nmo;
  GemmDesc g;
  g.M = nz; g.N = ncl; g.K = naux_w(c); g.nb1 = nr;
  g.A = gam; g.sAm = naux_w(c); g.sAk = 1;
  g.B = B + (long)r0 * nmo + c0; g.sBk = (long)nmo * nmo; g.sBn = 1; g.sBb1 = nmo;
  g.C = S; g.ldc = svS; g.sCb1 = ldS;
  g.alpha = coef; g.beta = 1.0;
  return gemm(c, g);
}

// accT_g[(j,x)][b] += coef * sum_P sum_{i,a} B[P][j][i] Zp_g[i][x][a] B[P][v0+a][v0+b]
static int exchange_main(xt_ctx* c, int nz, const DevBuf& B, double coef) {
  if (coef == 0.0) return 0;
  const int O = c->O, V = c->V, nmo = c->d.nmo, naux = naux_w(c);
  const long mm = (long)nmo * nmo, chs = (long)nz * O * V;
  if (naux <= 0) return 0;
  Group gr[2];
  const int ngr = channel_groups(c, gr);
  for (int q = 0; q < ngr; ++q) {
    const int nzg = gr[q].nch * nz;
    const size_t per = (size_t)O * nzg * V;
    int pc = (int)(chunk_budget(c, (size_t)3 << 30) / (8 * per));
    if (pc < 1) pc = 1;
    if (pc > naux) pc = naux;
    RET(c->tbuf.ensure((size_t)pc * per));
    const double* Bo = bmo_of(c, B, gr[q].ob);
    const double* Bv = bmo_of(c, B, gr[q].vb);
    const double* zp = c->zp.p + gr[q].ch0 * chs;
    double* at = c->accT.p + gr[q].ch0 * chs;
    for (int p0 = 0; p0 < naux; p0 += pc) {
      const int np = (p0 + pc <= naux) ? pc : naux - p0;
      GemmDesc g1;   // T[P] (O, nzg*V) = B[P][occ][occ] . Zp
      g1.M = O; g1.N = nzg * V; g1.K = O; g1.nb1 = np;
      g1.A = Bo + p0 * mm; g1.sAm = nmo; g1.sAk = 1; g1.sAb1 = mm;
      g1.B = zp; g1.sBk = (long)nzg * V; g1.sBn = 1;
      g1.C = c->tbuf.p; g1.ldc = (long)nzg * V; g1.sCb1 = (long)per;
      RET(gemm(c, g1));
      GemmDesc g2;   // accT[(j,x)][b] += coef * sum_{P,a} T[P][(j,x)][a] B[P][v0+a][v0+b]
      g2.M = O * nzg; g2.N = V; g2.K = V; g2.R = np;
      g2.A = c->tbuf.p; g2.sAm = V; g2.sAk = 1; g2.sAr = (long)per;
      g2.B = Bv + p0 * mm + (long)c->v0 * nmo + c->v0; g2.sBk = nmo; g2.sBn = 1; g2.sBr = mm;
      g2.C = at; g2.ldc = V;
      g2.alpha = coef; g2.beta = 1.0;
      g2.tag = 1;
      RET(gemm(c, g2));
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Stored MO exchange (XT_K_STORED).  Per channel group g (occupied basis ob,
// virtual basis vb) the exchange kernel of the sandwich above, contracted over
// P once per solve and kept in HBM:
//   Kx_g[(i,a),(j,b)] = ck sum_P Bo[P][i][j] Bv[P][v0+a][v0+b] + ck_lr (same, long range)
// (symmetric under (i,a) <-> (j,b); (O V)^2 doubles per group).  Per A.x the
// exchange is then one skinny GEMM  acc_g[x][(j,b)] -= sum_(i,a) Ze_g[x][(i,a)] Kx_g[(i,a),(j,b)],
// streaming Kx once (HBM-bound, 2 nzg flops per 8 bytes) instead of the
// 2 naux nzg O V^2 flops of the DF sandwich.  The reference makes the same
// trade when PySCF keeps the ERIs incore (mf._eri, max_memory) rather than
// running integral-direct J/K.
// ---------------------------------------------------------------------------
// row stride of the stored exchange: O V rounded up to 8 doubles (64 B) so every
// row starts 16-B aligned for the streaming kernel's wide loads
static size_t kx_ld(const xt_ctx* c) {
  const size_t ov = (size_t)c->O * c->V;
  return (ov + 7) & ~(size_t)7;
}

static size_t kx_doubles(const xt_ctx* c) {
  Group gr[2];
  const int ngr = channel_groups(c, gr);
  return (size_t)(krow1(c) - krow0(c)) * c->V * kx_ld(c) * (size_t)ngr;
}

static bool has_exchange(const xt_ctx* c) {
  return (c->ck != 0.0 || c->ck_lr != 0.0) && c->d.naux > 0;
}

extern "C" int xt_set_partition(xt_ctx* c, int p0, int p1, int i0, int i1) {
  if (!c) return fail(XT_ERR_ARG, "null ctx");
  if (c->trimmed) return fail(XT_ERR_STATE, "the MO factor was trimmed to this rank's aux window; set it again");
  if (p0 < 0 || p1 < p0 || p1 > c->d.naux) return fail(XT_ERR_ARG, "aux window outside [0, naux]");
  if (i0 < 0 || i1 < i0 || i1 > c->O) return fail(XT_ERR_ARG, "exchange rows outside [0, O]");
  c->win_p0 = p0; c->win_np = p1 - p0;
  c->kr0 = i0; c->kr1 = i1;
  c->kx_valid = false; c->k_resolved = -1;
  return 0;
}

static int resolve_kmode(xt_ctx* c) {
  if (c->k_resolved >= 0) return 0;
  if (!has_exchange(c) || c->kmode == XT_K_DIRECT) { c->k_resolved = 0; return 0; }
  if (c->kmode == XT_K_STORED) { c->k_resolved = 1; return 0; }
  const size_t need = kx_doubles(c) * 8;
  size_t cap;
  if (c->k_max_bytes > 0) {
    cap = (size_t)c->k_max_bytes;
  } else {
    size_t fr = 0, tot = 0;
    HIPCHK("", hipMemGetInfo(&fr, &tot));
    fr += c->Kx.n * 8;                       // an existing matrix would be reused
    size_t reserve = tot / 10;
    if (reserve < ((size_t)24 << 30)) reserve = (size_t)24 << 30;   // XC chunks, Davidson subspace
    cap = fr > reserve ? fr - reserve : 0;
  }
  c->k_resolved = need <= cap ? 1 : 0;
  return 0;
}

// occupied rows per stored-exchange build GEMM (the fold of the symmetric build, build_kx)
constexpr int KX_FOLD = 8;

static int build_kx(xt_ctx* c) {
  if (c->trimmed) return fail(XT_ERR_STATE, "the stored exchange needs every aux row: set the factor again");
  const int O = c->O, V = c->V, nmo = c->d.nmo, naux = c->d.naux;
  const long mm = (long)nmo * nmo;
  const size_t ov = (size_t)O * V, ld = kx_ld(c);
  const int i0 = krow0(c), i1 = krow1(c);
  const size_t blk = (size_t)(i1 - i0) * V * ld;   // this context's rows of one group
  Group gr[2];
  const int ngr = channel_groups(c, gr);
  if (blk == 0) { c->kx_valid = true; return 0; }
  // + zeroed slack rows after the last group (the streaming kernel's tail loads)
  RET(c->Kx.ensure(blk * ngr + (size_t)SKINNY_B_SLACK * ld));
  HIPCHK("", hipMemsetAsync(c->Kx.p, 0, c->Kx.n * 8, c->st));
  for (int q = 0; q < ngr; ++q) {
    double* K = c->Kx.p + (size_t)q * blk - (size_t)i0 * V * ld;   // row (i,a) at (i V + a) ld
    for (int pass = 0; pass < 2; ++pass) {
      const double coef = pass ? c->ck_lr : c->ck;
      if (coef == 0.0) continue;
      const DevBuf& B = pass ? c->Bmo_lr : c->Bmo;
      const double* Bo = bmo_full(c, B, gr[q].ob);   // all aux rows: Kx sums over every P
      const double* Bv = bmo_full(c, B, gr[q].vb) + (long)c->v0 * nmo + c->v0;
      // batch a: Kx[(i,a)][(j,b)] += coef sum_P Bo[P][i][j] Bv[P][a][b] with rows (i, j) of
      // a chunk of KX_FOLD occupied i in one GEMM (two-level rows: i strides nmo in Bo and
      // V ld in Kx, j strides 1 and V).  Kx is symmetric under (i,a) <-> (j,b), so a chunk
      // [ci, ce) computes only j >= ci (and the j < i0 outside this context's rows); the
      // blocks (i, j) with i0 <= j < ci are transposes of blocks built by earlier chunks
      // and are mirrored afterwards: ~54 % of the full build's flops at O = 101.
      for (int ci = i0; ci < i1; ci += KX_FOLD) {
        const int ce = ci + KX_FOLD < i1 ? ci + KX_FOLD : i1;
        const int jr[2][2] = {{0, i0}, {ci, O}};
        for (int r = 0; r < 2; ++r) {
          const int j0 = jr[r][0], j1 = jr[r][1];
          if (j1 <= j0) continue;
          GemmDesc g;
          g.M = (ce - ci) * (j1 - j0); g.N = V; g.K = naux; g.nb1 = V;
          g.rdiv = j1 - j0; g.sAm_hi = nmo; g.sC_hi = (long)V * ld;
          g.A = Bo + (long)ci * nmo + j0; g.sAm = 1; g.sAk = mm; g.sAb1 = 0;
          g.B = Bv; g.sBk = mm; g.sBn = 1; g.sBb1 = nmo;
          g.C = K + (size_t)ci * V * ld + (size_t)j0 * V; g.ldc = V; g.sCb1 = (long)ld;
          g.alpha = coef; g.beta = 1.0;
          RET(gemm(c, g));
        }
      }
    }
    kx_mirror(c->st, O, V, (long)ld, i0, i1, KX_FOLD, K);
    HIPCHK("", hipGetLastError());   // a rejected mirror launch would leave zero blocks in Kx
  }
  HIPCHK("", hipStreamSynchronize(c->st));
  c->kx_valid = true;
  return 0;
}

// C (M x ov) = alpha A Kx_rows + beta C through the skinny streaming kernel (xt_exch.hip),
// M <= SKINNY_MAX_M: one pass over the K = (i1 - i0) V stored rows at B, timed as tag 1
static int skinny_exchange(xt_ctx* c, int M, int K, double alpha, const double* A, const double* B, double beta,
                           double* C) {
  const size_t ov = (size_t)c->O * c->V;
  const size_t need = skinny_workspace_bytes(M, (int)ov, K);
  if (c->ws.n * sizeof(double) < need) RET(c->ws.ensure(need / sizeof(double) + 1));
  return profiled(c, 1, 2.0 * M * (double)ov * K, 8.0 * ((double)ov * K + (double)M * K + 2.0 * M * (double)ov),
                  "skinny exchange", [&] {
                    return skinny_gemm(M, (int)ov, K, alpha, A, (long)ov, B, (long)kx_ld(c), beta, C, (long)ov,
                                       c->ws.p, c->ws.n * sizeof(double), c->st);
                  });
}

// Per group: acc_g[x][(j,b)] -= sum_{(i,a), i in [i0,i1)} Ze_g[x][(i,a)] Kx_g[(i,a)][(j,b)].
// Up to SKINNY_MAX_M rows (2 nz <= 48: the headline's 40) the skinny streaming kernel
// (xt_exch.hip) reads Kx once with wide loads straight into the MFMA operands;
// more rows take the generic tile, which also reads Kx once.
static int exchange_stored(xt_ctx* c, int nz) {
  const size_t ov = (size_t)c->O * c->V, ld = kx_ld(c);
  const long chs = (long)nz * ov;
  const int i0 = krow0(c), i1 = krow1(c);
  const size_t blk = (size_t)(i1 - i0) * c->V * ld;
  if (blk == 0) return 0;
  Group gr[2];
  const int ngr = channel_groups(c, gr);
  for (int q = 0; q < ngr; ++q) {
    const int M = gr[q].nch * nz, K = (i1 - i0) * c->V;
    const double* A = c->ze.p + gr[q].ch0 * chs + (long)i0 * c->V;
    const double* B = c->Kx.p + (size_t)q * blk;
    double* C = c->acc.p + gr[q].ch0 * chs;
    if (M <= SKINNY_MAX_M) {
      RET(skinny_exchange(c, M, K, -1.0, A, B, 1.0, C));
      continue;
    }
    GemmDesc g;
    g.M = M; g.N = (int)ov; g.K = K;
    g.A = A; g.sAm = (long)ov; g.sAk = 1;
    g.B = B; g.sBk = (long)ld; g.sBn = 1;
    g.C = C; g.ldc = (long)ov;
    g.alpha = -1.0; g.beta = 1.0;
    g.tag = 1;
    RET(gemm(c, g));
  }
  return 0;
}

// XSF with spin adaptation SA >= 2 through the stored matrix: the main exchange
// (-Kx z) and the twelve Delta-A exchange projections (XSF_TDA.py:1175-1274, the
// direct sandwiches of xsf_delta_a) are all sub-blocks of Kx applied to the four
// source blocks of z, so ONE stream of Kx with the four blocks as 4 nz rows gives
// every term; a 4 x 4 weight table (source block, target block) combines them.
// Kx carries c_K: the Delta-A coefficients (on sum_P B B) are divided by it.
static bool xsf_fused_k(const xt_ctx* c) {
  const xt_desc& d = c->d;
  return d.kind == XT_KIND_XSF && d.sa > 1 && c->k_resolved == 1 && c->ck != 0.0 && c->ck_lr == 0.0 &&
         c->nchan == 1;
}

// the XSF Delta-A coefficients (XSF_TDA.py:1175-1274) of a descriptor, S = no / 2: read by
// xsf_delta_a and by the weight table of exchange_stored_xsf, which must agree
struct XsfFactors {
  double si, fg, ff, tsm1, f1, f2, f3, f4;
  explicit XsfFactors(const xt_desc& d) {
    si = d.no / 2.0;
    fg = d.fglobal; ff = fg * d.foo;
    tsm1 = 2 * si - 1;
    f1 = sqrt((2 * si + 1) / (2 * si)) - 1;
    f2 = sqrt((2 * si + 1) / (2 * si - 1));
    f3 = sqrt((2 * si) / (2 * si - 1)) - 1;
    f4 = 1 / sqrt(2 * si * (2 * si - 1));
  }
};

static int exchange_stored_xsf(xt_ctx* c, int nz) {
  const xt_desc& d = c->d;
  const int O = c->O, V = c->V, nc = d.nc, no = d.no;
  const size_t ov = (size_t)O * V, ld = kx_ld(c);
  const int i0 = krow0(c), i1 = krow1(c);
  const size_t blk = (size_t)(i1 - i0) * V * ld;
  if (blk == 0) return 0;
  const int K = (i1 - i0) * V;
  const int zmax = SKINNY_MAX_M / 4;           // trial vectors per Kx stream
  // coefficient table (xsf_delta_a's sandwich coefficients / c_K), source X -> target Y
  const XsfFactors xf(d);
  const double fg = xf.fg, ff = xf.ff, tsm1 = xf.tsm1, f1 = xf.f1, f2 = xf.f2, f3 = xf.f3;
  enum { CV = 0, CO = 1, OV = 2, OO = 3 };
  double dk[4][4] = {};
  dk[CO][CV] = dk[CV][CO] = dk[OV][CV] = dk[CV][OV] = -fg * f1;   // cv_co, co_cv, cv_ov, ov_cv
  dk[OV][CO] = dk[CO][OV] = -fg / tsm1;                           // co_ov, ov_co
  if (d.sa > 2) {
    dk[OO][CV] = dk[CV][OO] = -ff * (f2 - 1);                     // cv_oo, oo_cv
    dk[OO][CO] = dk[CO][OO] = dk[OO][OV] = dk[OV][OO] = -ff * f3; // co_oo, oo_co, ov_oo, oo_ov
  }
  W16 w;
  for (int X = 0; X < 4; ++X)
    for (int Y = 0; Y < 4; ++Y) w.w[4 * X + Y] = -1.0 + dk[X][Y] / c->ck;   // main exchange: -Kx z
  for (int z0 = 0; z0 < nz; z0 += zmax) {
    const int nzb = nz - z0 < zmax ? nz - z0 : zmax, M = 4 * nzb;
    RET(c->zr.ensure((size_t)M * ov));
    RET(c->tbuf.ensure((size_t)M * ov));
    xsf_split4(c->st, nzb, O, V, nc, no, c->ze.p + (size_t)z0 * ov, c->zr.p);
    RET(skinny_exchange(c, M, K, 1.0, c->zr.p + (long)i0 * V, c->Kx.p, 0.0, c->tbuf.p));
    xsf_combine4(c->st, nzb, O, V, nc, no, w, c->tbuf.p, c->acc.p + (size_t)z0 * ov);
  }
  return 0;
}

extern "C" int xt_set_exchange_mode(xt_ctx* c, int mode, double max_gib) {
  if (!c) return fail(XT_ERR_ARG, "null ctx");
  if (mode < XT_K_AUTO || mode > XT_K_STORED) return fail(XT_ERR_ARG, "bad exchange mode");
  c->kmode = mode;
  c->k_max_bytes = max_gib > 0 ? max_gib * (double)((size_t)1 << 30) : 0.0;
  c->k_resolved = -1;
  if (mode == XT_K_DIRECT) { c->Kx.release(); c->kx_valid = false; }
  return 0;
}

extern "C" int xt_exchange_plan(xt_ctx* c, int* stored, double* k_gib) {
  if (!c) return fail(XT_ERR_ARG, "null ctx");
  (void)hipSetDevice(c->d.device);
  RET(resolve_kmode(c));
  if (stored) *stored = c->k_resolved == 1 ? 1 : 0;
  if (k_gib) *k_gib = has_exchange(c) ? kx_doubles(c) * 8.0 / (double)((size_t)1 << 30) : 0.0;
  return 0;
}

// Once a partitioned context holds its rows of the stored exchange, only the aux window
// [win_p0, win_p0 + win_np) of the MO factor is ever read again (J, the XSF Delta-A, the
// preconditioner diagonals): the other rows are dropped, so a replicated factor costs
// naux / N rows per rank instead of naux (24 GB -> 3 GB at the headline, N = 8).
static int trim_factor(xt_ctx* c) {
  const int np = c->win_np, p0 = c->win_p0, naux = c->d.naux;
  DevBuf* bufs[2] = {&c->Bmo, &c->Bmo_lr};
  for (DevBuf* B : bufs)
    if (B->p) RET(relay_factor(c, *B, naux, p0, np, np));   // B takes the window, the full factor is freed
  c->naux_full = naux;
  c->d.naux = np;
  c->win_p0 = 0; c->win_np = -1;
  c->trimmed = true;
  return 0;
}

extern "C" int xt_prepare(xt_ctx* c, int* k_mode, double* k_gib) {
  if (!c) return fail(XT_ERR_ARG, "null ctx");
  (void)hipSetDevice(c->d.device);
  if (has_exchange(c) && !c->has_df) return fail(XT_ERR_STATE, "DF factor not set");
  RET(resolve_kmode(c));
  if (c->k_resolved == 1 && !c->kx_valid) RET(build_kx(c));
  if (c->k_resolved == 1 && c->kx_valid && c->win_np > 0 && c->win_np < c->d.naux) RET(trim_factor(c));
  if (k_mode) *k_mode = c->k_resolved == 1 ? XT_K_STORED : XT_K_DIRECT;
  if (k_gib) *k_gib = c->k_resolved == 1 ? kx_doubles(c) * 8.0 / (double)((size_t)1 << 30) : 0.0;
  return 0;
}

// ---------------------------------------------------------------------------
// XSF spin-adaptation Delta-A (XSF_TDA.py:1175-1274), ROKS only
// full-space blocks: rows [0,nc) core / [nc,O) open ; cols [0,no) open / [no,V) virtual
// ---------------------------------------------------------------------------
static int xsf_delta_a(xt_ctx* c, int nz, bool skip_k) {
  const xt_desc& d = c->d;
  const int nc = d.nc, no = d.no, nv = d.nv, O = c->O, V = c->V, nmo = d.nmo;
  const long ld = V, sv = (long)O * V, mm = (long)nmo * nmo;
  const XsfFactors xf(d);
  const double si = xf.si, fg = xf.fg, ff = xf.ff, tsm1 = xf.tsm1, f1 = xf.f1, f2 = xf.f2, f3 = xf.f3, f4 = xf.f4;
  const double* Z = c->ze.p;
  double* S = c->acc.p;
  // block pointers in the full space
  const double* Zcv = Z + no;            double* Scv = S + no;
  const double* Zco = Z;                 double* Sco = S;
  const double* Zov = Z + nc * ld + no;  double* Sov = S + nc * ld + no;
  const double* Zoo = Z + nc * ld;       double* Soo = S + nc * ld;
  const double* FAh = c->F.p + 2 * mm;
  const double* FBh = c->F.p + 3 * mm;
  const double* FS = c->F.p + 4 * mm;
  // MO offsets
  const int mc = 0, mo_ = nc, mv = nc + no;
  const bool loc = d.add_local != 0;
  if (loc) {
    // SA >= 1 one-electron parts
    RET(right_mo(c, nz, nc, nv, nv, Zcv, ld, sv, FS + (long)mv * nmo + mv, nmo, 1, Scv, ld, sv, fg / si));
    RET(left_mo(c, nz, nc, nc, nv, FS + (long)mc * nmo + mc, 1, nmo, Zcv, ld, sv, Scv, ld, sv, fg / si));
    RET(left_mo(c, nz, nc, nc, no, FS, 1, nmo, Zco, ld, sv, Sco, ld, sv, fg * 2.0 / tsm1));
    RET(right_mo(c, nz, no, nv, nv, Zov, ld, sv, FS + (long)mv * nmo + mv, nmo, 1, Sov, ld, sv, fg * 2.0 / tsm1));
  }
  const double* B = bmo_of(c, c->Bmo, 0);
  // J parts: gamma_co, gamma_ov
  RET(c->gam.ensure((size_t)nz * naux_w(c) + 1));
  RET(c->gam2.ensure((size_t)nz * naux_w(c) + 1));
  RET(coulomb_gamma(c, B, nz, mc, nc, mo_, no, Zco, ld, sv, c->gam.p, 0.0));
  RET(coulomb_gamma(c, B, nz, mo_, no, mv, nv, Zov, ld, sv, c->gam2.p, 0.0));
  RET(coulomb_project(c, B, nz, mc, nc, mo_, no, c->gam.p, Sco, ld, sv, -fg / tsm1));
  RET(coulomb_project(c, B, nz, mo_, no, mv, nv, c->gam2.p, Sov, ld, sv, -fg / tsm1));
  if (d.sa > 1) {
    RET(coulomb_project(c, B, nz, mc, nc, mo_, no, c->gam2.p, Sco, ld, sv, fg / tsm1));   // co_ov_j
    RET(coulomb_project(c, B, nz, mo_, no, mv, nv, c->gam.p, Sov, ld, sv, fg / tsm1));   // ov_co_j
    if (loc) {
      // fB_vo = FBh[mv+a][mo_+v] ; fA_oc = FAh[mo_+v][mc+i]
      RET(right_mo(c, nz, nc, no, nv, Zco, ld, sv, FBh + (long)mv * nmo + mo_, 1, nmo, Scv, ld, sv, fg * f1));
      RET(right_mo(c, nz, nc, nv, no, Zcv, ld, sv, FBh + (long)mv * nmo + mo_, nmo, 1, Sco, ld, sv, fg * f1));
      RET(left_mo(c, nz, nc, no, nv, FAh + (long)mo_ * nmo + mc, 1, nmo, Zov, ld, sv, Scv, ld, sv, -fg * f1));
      RET(left_mo(c, nz, no, nc, nv, FAh + (long)mo_ * nmo + mc, nmo, 1, Zcv, ld, sv, Sov, ld, sv, -fg * f1));
    }
    // K parts: S_Y += coef * sum_P B[rowsY,rowsX] Z_X B[colsX,colsY]
    // (skip_k: applied through the stored exchange matrix, exchange_stored_xsf)
    // blocks: cv (rows mc:nc, cols mv:nv) co (mc:nc, mo_:no) ov (mo_:no, mv:nv) oo (mo_:no, mo_:no)
    if (!skip_k) {
    RET(sandwich(c, B, B, nz, mc, nc, mc, nc, mo_, no, mv, nv, Zco, ld, sv, Scv, ld, sv, -fg * f1));   // cv_co_k
    RET(sandwich(c, B, B, nz, mc, nc, mc, nc, mv, nv, mo_, no, Zcv, ld, sv, Sco, ld, sv, -fg * f1));   // co_cv_k
    RET(sandwich(c, B, B, nz, mc, nc, mo_, no, mv, nv, mv, nv, Zov, ld, sv, Scv, ld, sv, -fg * f1));   // cv_ov_k
    RET(sandwich(c, B, B, nz, mo_, no, mc, nc, mv, nv, mv, nv, Zcv, ld, sv, Sov, ld, sv, -fg * f1));   // ov_cv_k
    RET(sandwich(c, B, B, nz, mc, nc, mo_, no, mv, nv, mo_, no, Zov, ld, sv, Sco, ld, sv, -fg / tsm1)); // co_ov_k
    RET(sandwich(c, B, B, nz, mo_, no, mc, nc, mo_, no, mv, nv, Zco, ld, sv, Sov, ld, sv, -fg / tsm1)); // ov_co_k
    }
  }
  if (d.sa > 2) {
    if (!skip_k) {
    RET(sandwich(c, B, B, nz, mc, nc, mo_, no, mo_, no, mv, nv, Zoo, ld, sv, Scv, ld, sv, -ff * (f2 - 1)));  // cv_oo_k
    RET(sandwich(c, B, B, nz, mo_, no, mc, nc, mv, nv, mo_, no, Zcv, ld, sv, Soo, ld, sv, -ff * (f2 - 1)));  // oo_cv_k
    RET(sandwich(c, B, B, nz, mc, nc, mo_, no, mo_, no, mo_, no, Zoo, ld, sv, Sco, ld, sv, -ff * f3));       // co_oo_k
    RET(sandwich(c, B, B, nz, mo_, no, mc, nc, mo_, no, mo_, no, Zco, ld, sv, Soo, ld, sv, -ff * f3));       // oo_co_k
    RET(sandwich(c, B, B, nz, mc + nc, no, mo_, no, mo_, no, mv, nv, Zoo, ld, sv, Sov, ld, sv, -ff * f3));   // ov_oo_k
    RET(sandwich(c, B, B, nz, mo_, no, mo_, no, mv, nv, mo_, no, Zov, ld, sv, Soo, ld, sv, -ff * f3));       // oo_ov_k
    }
    if (loc) {
      // fA_co = FAh[mc+i][mo_+w] ; fB_vo = FBh[mv+a][mo_+v]
      RET(left_mo(c, nz, nc, no, no, FAh + (long)mc * nmo + mo_, nmo, 1, Zoo, ld, sv, Sco, ld, sv, -ff * f3));
      RET(left_mo(c, nz, no, nc, no, FAh + (long)mc * nmo + mo_, 1, nmo, Zco, ld, sv, Soo, ld, sv, -ff * f3));
      RET(right_mo(c, nz, no, no, nv, Zoo, ld, sv, FBh + (long)mv * nmo + mo_, 1, nmo, Sov, ld, sv, ff * f3));
      RET(right_mo(c, nz, no, nv, no, Zov, ld, sv, FBh + (long)mv * nmo + mo_, nmo, 1, Soo, ld, sv, ff * f3));
      // trace / rank-one terms (XSF_TDA.py:1237-1269: 'xvv', 'vw,..' contractions)
      xsf_rank1(c->st, nz, nc, no, nv, nmo, ff * (f2 / si), ff * f4, Z, FS, FAh, FBh, S);
    }
  }
  return 0;
}

// the Coulomb / exchange response of xt_apply (d.naux > 0): J, -K (stored or direct), XSF Delta-A
int xt::jk_response(xt_ctx* c, int nz) {
  const xt_desc& d = c->d;
  const int O = c->O, V = c->V, nch = c->nchan;
  const long chs = (long)nz * O * V;
  const bool has_k = (c->ck != 0.0 || c->ck_lr != 0.0);
  bool xsf_k_done = false;   // Delta-A exchange already applied through the stored matrix
  if (!is_sf(d) && naux_w(c) > 0) {   // J (spin-conserving only)
    RET(c->gam.ensure((size_t)nz * naux_w(c)));
    for (int ch = 0; ch < nch; ++ch)
      RET(coulomb_gamma(c, bmo_of(c, c->Bmo, c->occ_basis[ch]), nz, 0, O, c->v0, V,
                        c->ze.p + ch * chs, V, (long)O * V, c->gam.p, ch == 0 ? 0.0 : 1.0));
    for (int ch = 0; ch < nch; ++ch)
      RET(coulomb_project(c, bmo_of(c, c->Bmo, c->occ_basis[ch]), nz, 0, O, c->v0, V, c->gam.p,
                          c->acc.p + ch * chs, V, (long)O * V, 1.0));
  }
  if (has_k) {
    RET(resolve_kmode(c));
    if (c->k_resolved == 1) {
      if (!c->kx_valid) RET(build_kx(c));
      if (xsf_fused_k(c)) {
        RET(exchange_stored_xsf(c, nz));
        xsf_k_done = true;
      } else {
        RET(exchange_stored(c, nz));
      }
    } else {
      RET(exchange_main(c, nz, c->Bmo, -c->ck));
      if (c->ck_lr != 0.0) RET(exchange_main(c, nz, c->Bmo_lr, -c->ck_lr));
    }
  }
  if (d.kind == XT_KIND_XSF && d.sa > 0 && naux_w(c) > 0) RET(xsf_delta_a(c, nz, xsf_k_done));
  return 0;
}

extern "C" int xt_xsf_j_diagonals(xt_ctx* c, double* co_j, double* ov_j, int ptr_kind) {
  if (!c || !co_j || !ov_j) return fail(XT_ERR_ARG, "null argument");
  if (!c->has_df) return fail(XT_ERR_STATE, "DF factor not set");
  (void)hipSetDevice(c->d.device);
  const int nc = c->d.nc, no = c->d.no, nv = c->d.nv;
  RET(c->trace.ensure((size_t)nc * no + (size_t)no * nv));
  // over this context's aux window (xt_set_partition): partial sums over ranks add up
  xsf_jdiag(c->st, naux_w(c), c->d.nmo, nc, no, nv, bmo_of(c, c->Bmo, 0), c->trace.p, c->trace.p + (size_t)nc * no);
  const hipMemcpyKind k = ptr_kind == XT_PTR_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  HIPCHK("", hipMemcpyAsync(co_j, c->trace.p, (size_t)nc * no * 8, k, c->st));
  HIPCHK("", hipMemcpyAsync(ov_j, c->trace.p + (size_t)nc * no, (size_t)no * nv * 8, k, c->st));
  HIPCHK("", hipStreamSynchronize(c->st));
  return 0;
}
