// xt_ctx_xc: the grid part of the operator context -- everything that knows the layout of
// the MO values on the two grids and of the weighted kernel:
//   Phi[b][c][g][p]     (nbasis, ncomp, ngrid, nmo) + XC_GRID_SLACK zeroed rows
//   nlcPhi[b][c][g][p]  (nbasis, 4, nlc_ng, nmo) on the VV10 grid
//   kern                the weighted fxc (or spin-flip kernel) per grid point
#include <hip/hip_runtime.h>
#include "xt_ctx.h"
#include "xt_kernels.h"

using namespace xt;

// dst[b][comp][g][p] = sum_mu ao[comp][g][mu] C_b[mu][p]: the AO values of ncomp planes of ng
// points projected on every MO basis, in chunks of points so that host inputs stream
// through c->stage (released by the caller after its synchronise)
static int project_ao(xt_ctx* c, const double* ao, int ncomp, int ng, double* dst, int ptr_kind) {
  const int nao = c->d.nao, nmo = c->d.nmo;
  const size_t gchunk_max = chunk_budget(c, (size_t)1 << 30) / (8 * (size_t)nao);
  int gc = (int)(gchunk_max < (size_t)ng ? gchunk_max : ng);
  if (gc < 1) gc = 1;
  if (ptr_kind == XT_PTR_HOST) RET(c->stage.ensure((size_t)gc * nao));
  for (int comp = 0; comp < ncomp; ++comp) {
    for (int g0 = 0; g0 < ng; g0 += gc) {
      const int n = (g0 + gc <= ng) ? gc : ng - g0;
      const double* src = ao + ((size_t)comp * ng + g0) * nao;
      if (ptr_kind == XT_PTR_HOST) {
        HIPCHK("", hipMemcpyAsync(c->stage.p, src, (size_t)n * nao * 8, hipMemcpyHostToDevice, c->st));
        src = c->stage.p;
      }
      for (int b = 0; b < c->nbasis; ++b) {
        GemmDesc g;
        g.M = n; g.N = nmo; g.K = nao;
        g.A = src; g.sAm = nao; g.sAk = 1;
        g.B = c->C.p + (size_t)b * nao * nmo; g.sBk = nmo; g.sBn = 1;
        g.C = dst + (((size_t)b * ncomp + comp) * ng + g0) * nmo; g.ldc = nmo;
        RET(gemm(c, g));
      }
    }
  }
  return 0;
}

// grid points per chunk of a response loop that holds per_g doubles per point: the byte
// budget over 8 per_g, at most ng, at least 64 (or ng)
static size_t grid_chunk(const xt_ctx* c, size_t default_budget, size_t per_g, int ng) {
  size_t G = chunk_budget(c, default_budget) / (8 * per_g);
  if (G > (size_t)ng) G = ng;
  if (G < 64) G = 64 < (size_t)ng ? 64 : ng;
  return G;
}

extern "C" int xt_set_grid(xt_ctx* c, const double* ao, const double* w, const double* kernel, int ptr_kind) {
  if (!c || !ao || !w || !kernel) return fail(XT_ERR_ARG, "null argument");
  if (!c->has_orb) return fail(XT_ERR_STATE, "xt_set_orbitals must precede xt_set_grid");
  (void)hipSetDevice(c->d.device);
  const int nmo = c->d.nmo, ng = c->d.ngrid;
  const bool sf = is_sf(c->d);
  // input ao carries c->ncomp components (1 for the density-only ALDA0 spin-flip kernel)
  const int ncomp = c->ncomp;
  // + zeroed slack rows after the last plane (fused XC kernels read whole K-tiles)
  const size_t phi_used = (size_t)c->nbasis * ncomp * ng * nmo;
  RET(c->Phi.ensure(phi_used + (size_t)XC_GRID_SLACK * nmo));
  HIPCHK("", hipMemsetAsync(c->Phi.p + phi_used, 0, (c->Phi.n - phi_used) * sizeof(double), c->st));
  RET(project_ao(c, ao, ncomp, ng, c->Phi.p, ptr_kind));
  if (sf && c->d.sf_kernel == XT_SF_ALDA0) {
    RET(to_device(c, c->kern, kernel, (size_t)ng, ptr_kind));   // already weighted
  } else {
    // UKS fxc (2, nk, 2, nk) x w, or the multicollinear spin-flip kernel (nk, nk) x 2 w
    const size_t n4 = (size_t)(sf ? 1 : 4) * c->nkc * c->nkc;
    RET(to_device(c, c->kern, kernel, n4 * ng, ptr_kind));
    RET(to_device(c, c->stage2, w, (size_t)ng, ptr_kind));
    weight_fxc(c->st, (long)n4, ng, sf ? 2.0 : 1.0, c->stage2.p, c->kern.p);
  }
  HIPCHK("", hipStreamSynchronize(c->st));
  c->stage.release(); c->stage2.release();
  c->has_grid = true;
  return 0;
}

extern "C" int xt_set_nlc(xt_ctx* c, int ng, const double* ao, const double* coords, const double* w, double b, double C,
                          double rho_min, int ptr_kind) {
  if (!c || !ao || !coords || !w) return fail(XT_ERR_ARG, "null argument");
  if (c->d.kind != XT_KIND_XTDA && c->d.kind != XT_KIND_UTDA)
    return fail(XT_ERR_ARG, "the VV10 response exists for XTDA / UTDA only (XTDA.py:515-517)");
  if (ng <= 0 || !(b > 0.0) || !(C >= 0.0) || !(rho_min >= 0.0))
    return fail(XT_ERR_ARG, "xt_set_nlc: need ngrid_nlc > 0, b > 0, C >= 0, rho_min >= 0");
  if (!c->has_orb) return fail(XT_ERR_STATE, "xt_set_orbitals must precede xt_set_nlc");
  (void)hipSetDevice(c->d.device);
  c->has_nlc = false;
  const int nmo = c->d.nmo;
  c->nlc_ng = ng; c->nlc_b = b; c->nlc_C = C; c->nlc_rho_min = rho_min;
  RET(c->nlcPhi.ensure((size_t)c->nbasis * 4 * ng * nmo));
  RET(c->nlcG.ensure((size_t)(3 + NLC_PLANES) * ng));
  RET(to_device(c, nlc_xyz(c), coords, (size_t)3 * ng, ptr_kind));
  RET(to_device(c, nlc_plane(c, NLC_W), w, (size_t)ng, ptr_kind));
  RET(project_ao(c, ao, 4, ng, c->nlcPhi.p, ptr_kind));
  const long compP = (long)ng * nmo;
  const double* PA = c->nlcPhi.p;
  const double* PB = c->nlcPhi.p + (size_t)c->occ_basis[1] * 4 * compP;
  vv10_rho0(c->st, ng, nmo, compP, PA, c->d.nc + c->d.no, PB, c->d.nc, nlc_plane(c, NLC_RHO),
            nlc_plane(c, NLC_GRAD), nlc_plane(c, NLC_GAM));
  RET(xt_vv10_ground(ng, nlc_xyz(c), nlc_plane(c, NLC_W), nlc_plane(c, NLC_RHO), nlc_plane(c, NLC_GAM), b, C,
                     rho_min, 0, ng, nlc_plane(c, NLC_SUMS), c->st));
  vv10_vgamma0(c->st, ng, nlc_plane(c, NLC_W), nlc_plane(c, NLC_RHO), nlc_plane(c, NLC_GAM),
               nlc_plane(c, NLC_SUMS), b, C, rho_min, nlc_plane(c, NLC_VG));
  HIPCHK("", hipStreamSynchronize(c->st));
  c->stage.release();
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(XT_ERR_HIP, std::string("xt_set_nlc kernel error: ") + hipGetErrorString(e));
  c->has_nlc = true;
  return 0;
}

// ---------------------------------------------------------------------------
// XC response over the grid (chunks of G points), W route (see k_xc_uks_w):
//   F1  U = PhiV0 Ze^T                              (GEMM, tag 2)
//   F2' rhoW[g][xg][c] = sum_a (PhiO0 Zp)[g,xg,a] dPhiV_c[g,a]
//                                                   (fused GEMM mode 1, tag 4: W never stored)
//   point kernel: rho = U-part + rhoW; wv; U <- L; rhoW <- wv[1..3]
//   B1  acc += L^T PhiV0                            (GEMM, tag 3)
//   B2' accT += PhiO0^T M, M[g,xg,a] = sum_c wv_c dPhiV_c[g,a] generated on the fly
//                                                   (fused GEMM mode 2, tag 5: M never stored)
// LDA / ALDA0: F1, point kernel, B1.
// ---------------------------------------------------------------------------
int xt::xc_response(xt_ctx* c, int nz) {
  const int O = c->O, V = c->V, nmo = c->d.nmo, ng = c->d.ngrid, nc = c->ncomp;
  const int nch = c->nchan;
  const bool gga = (nc == 4);
  const bool mgga = (c->nkc == 5);
  const long chs = (long)nz * O * V;
  Group gr[2];
  const int ngr = channel_groups(c, gr);
  const size_t per_g = (size_t)nch * nz * O * (mgga ? 4 : 1) + (gga ? (size_t)nch * nz * 3 : 0);
  const size_t G = grid_chunk(c, (size_t)8 << 30, per_g, ng);
  RET(c->ubuf.ensure((size_t)nch * nz * O * G));
  if (gga) RET(c->wbuf.ensure((size_t)nch * nz * 3 * (G + XC_GRID_SLACK)));
  // MGGA: three tau planes T_c = dPhiV_c Ze^T laid out like U (forward), then the tau
  // potential's back operands 1/2 wv_tau dPhiO_c (point kernel)
  if (mgga) RET(c->taubuf.ensure((size_t)3 * nch * nz * O * G));
  const long compP = (long)ng * nmo;
  const long basP = (long)nc * compP;
  const int nab = (V + 15) / 16;
  for (int g0 = 0; g0 < ng; g0 += (int)G) {
    const int n = (g0 + (int)G <= ng) ? (int)G : ng - g0;
    double* Ug[2]; double* Rg[2]; long ldU[2], ldR[2];
    for (int q = 0; q < ngr; ++q) {
      const int nzg = gr[q].nch * nz;
      Ug[q] = c->ubuf.p + (long)gr[q].ch0 * nz * O * n;  ldU[q] = (long)nzg * O;
      // each group's wv block is followed by XC_GRID_SLACK zero rows (the M-backward
      // kernel's last K-tile reads them instead of masking rows past n)
      Rg[q] = gga ? c->wbuf.p + (long)gr[q].ch0 * nz * 3 * (n + XC_GRID_SLACK) : nullptr;  ldR[q] = (long)nzg * 3;
      if (gga && hipMemsetAsync(Rg[q] + (long)n * ldR[q], 0, sizeof(double) * XC_GRID_SLACK * ldR[q], c->st) !=
                     hipSuccess)
        return fail(XT_ERR_HIP, "wv slack memset failed");
      const double* PV = c->Phi.p + gr[q].vb * basP + (long)g0 * nmo + c->v0;
      const double* PO = c->Phi.p + gr[q].ob * basP + (long)g0 * nmo;
      GemmDesc f1;   // U[g][(x,i)] = sum_a PhiV0[g][a] Ze[(x,i)][a]
      f1.M = n; f1.N = nzg * O; f1.K = V;
      f1.A = PV; f1.sAm = nmo; f1.sAk = 1;
      f1.B = c->ze.p + gr[q].ch0 * chs; f1.sBn = V; f1.sBk = 1;
      f1.C = Ug[q]; f1.ldc = ldU[q];
      f1.tag = 2;
      RET(gemm(c, f1));
      if (mgga) {
        const long tcs = (long)nch * nz * O * n;
        for (int cc = 1; cc < 4; ++cc) {   // T_c[g][(x,i)] = sum_a dPhiV_c[g][a] Ze[(x,i)][a]
          GemmDesc ft = f1;
          ft.A = PV + cc * compP;
          ft.C = c->taubuf.p + (cc - 1) * tcs + (long)gr[q].ch0 * nz * O * n;
          RET(gemm(c, ft));
        }
      }
      // the dedicated kernel pays off from ~5 occupied 16-row blocks up (O = 101: 168.6 vs
      // 173.1 ms/step; O = 91, C3mc: 75.2 vs 87.0; O = 34 / 37: 18 % / 15 % slower than the
      // engine's mode 1, and the small-O kernel takes O <= 48)
      const bool w_ded = c->w_kernel == 1 || (c->w_kernel == 2 && O > 64);
      const bool w_small = (c->w_kernel == 3 || (c->w_kernel == 2 && nzg >= 8)) &&
                           xc_rho_ws_lds_bytes(O) <= 160 * 1024;
      // tag 4 cost of this group's rho-forward, whichever kernel runs it.  flops: the T = PhiO^T Zp
      // GEMM (2 O per T element) + the fused gradient contraction rhoW = sum_a dPhiV_c T (3 FMAs
      // per T element); bytes: Zp, PhiO0, dPhiV_{x,y,z} in, rhoW out
      const double w_flops = 2.0 * nzg * V * (double)n * (O + 3);
      const double w_bytes = 8.0 * ((double)nzg * O * V + (double)n * O + 3.0 * n * V + 3.0 * n * nzg);
      const double* Zp = c->zp.p + gr[q].ch0 * chs;
      if (gga && w_small) {
        // small-O kernel (xt_xcws.hip): every pair of a 64-point block, weights staged once
        RET(profiled(c, 4, w_flops, w_bytes, "xc_rho_ws", [&] {
          return xc_rho_ws(O, nzg, V, n, PO, nmo, Zp, (long)nzg * V, V, PV + compP, compP, nmo, Rg[q], ldR[q], c->st);
        }));
      } else if (gga && w_ded && xc_rho_w_lds_bytes(O) <= 160 * 1024) {
        // dedicated kernel (xt_xcw.hip); tag 4 timing
        RET(profiled(c, 4, w_flops, w_bytes, "xc_rho_w", [&] {
          return xc_rho_w(O, nzg, V, n, PO, nmo, Zp, (long)nzg * V, V, PV + compP, compP, nmo, Rg[q], ldR[q], c->st);
        }));
      } else if (gga) {
        GemmDesc f2;   // rhoW[g][xg][c] = sum_a sum_i PhiO0[g][i] Zp[i][xg][a] dPhiV_c[g][a]
        f2.M = 16 * nzg; f2.N = n; f2.K = O; f2.R = nab;
        f2.A = Zp; f2.sAm = 1; f2.sAk = (long)nzg * V; f2.sAr = 16;
        f2.B = PO; f2.sBk = 1; f2.sBn = nmo;
        f2.fz.mode = 1; f2.fz.ablk = V; f2.fz.V = V; f2.fz.nx = nzg;
        f2.fz.w = PV + compP; f2.fz.wc = compP; f2.fz.wg = nmo;
        f2.fz.rho = Rg[q]; f2.fz.rg = ldR[q];
        f2.tag = 4;
        f2.flops = w_flops; f2.bytes = w_bytes;
        RET(gemm(c, f2));
      }
    }
    if (nch == 2) {
      // spin s -> (group, row offset inside the group)
      double* Us[2]; double* Rs[2]; long lus[2], lrs[2];
      for (int s = 0; s < 2; ++s) {
        const int q = (ngr == 1) ? 0 : s;
        const int off = (ngr == 1) ? s : 0;
        Us[s] = Ug[q] + (long)off * nz * O; lus[s] = ldU[q];
        Rs[s] = gga ? Rg[q] + (long)off * nz * 3 : nullptr; lrs[s] = ldR[q];
      }
      if (mgga) {
        double* Ts[2];
        for (int s = 0; s < 2; ++s) Ts[s] = c->taubuf.p + (Us[s] - c->ubuf.p);   // same layout as U
        xc_uks_mgga(c->st, 2, n, g0, ng, nz, O, nmo, compP, c->Phi.p + c->occ_basis[0] * basP,
                    c->Phi.p + c->occ_basis[1] * basP, c->kern.p, Us[0], lus[0], Us[1], lus[1], Ts[0], Ts[1],
                    (long)nch * nz * O * n, Rs[0], lrs[0], Rs[1], lrs[1]);
      } else {
        xc_uks_w(c->st, 2, nc, n, g0, ng, nz, O, nmo, compP,
                 c->Phi.p + c->occ_basis[0] * basP, c->Phi.p + c->occ_basis[1] * basP,
                 c->kern.p, Us[0], lus[0], Us[1], lus[1], Rs[0], lrs[0], Rs[1], lrs[1]);
      }
    } else if (mgga) {   // one spin-flip channel, multicollinear (rho, grad rho, tau) kernel
      xc_uks_mgga(c->st, 1, n, g0, ng, nz, O, nmo, compP, c->Phi.p + c->occ_basis[0] * basP, nullptr, c->kern.p,
                  Ug[0], ldU[0], nullptr, 0, c->taubuf.p, nullptr, (long)nz * O * n, Rg[0], ldR[0], nullptr, 0);
    } else if (gga) {    // one spin-flip channel, multicollinear (rho, grad rho) kernel
      xc_uks_w(c->st, 1, nc, n, g0, ng, nz, O, nmo, compP, c->Phi.p + c->occ_basis[0] * basP, nullptr, c->kern.p,
               Ug[0], ldU[0], nullptr, 0, Rg[0], ldR[0], nullptr, 0);
    } else {             // ALDA0, or the multicollinear LDA kernel (2 w f_ss: scalar)
      xc_sf(c->st, n, g0, nz, O, nmo, c->Phi.p + c->occ_basis[0] * basP, c->kern.p, Ug[0]);
    }
    for (int q = 0; q < ngr; ++q) {
      const int nzg = gr[q].nch * nz;
      const double* PV = c->Phi.p + gr[q].vb * basP + (long)g0 * nmo + c->v0;
      const double* PO = c->Phi.p + gr[q].ob * basP + (long)g0 * nmo;
      GemmDesc b1;   // acc[(x,i)][a] += sum_g L[g][(x,i)] PhiV0[g][a]
      b1.M = nzg * O; b1.N = V; b1.K = n;
      b1.A = Ug[q]; b1.sAm = 1; b1.sAk = ldU[q];
      b1.B = PV; b1.sBk = nmo; b1.sBn = 1;
      b1.C = c->acc.p + gr[q].ch0 * chs; b1.ldc = V; b1.beta = 1.0;
      b1.tag = 3;
      RET(gemm(c, b1));
      if (mgga) {
        const long tcs = (long)nch * nz * O * n;
        for (int cc = 1; cc < 4; ++cc) {   // acc[(x,i)][a] += sum_g (1/2 wv_tau dPhiO_c)[g][(x,i)] dPhiV_c[g][a]
          GemmDesc bt = b1;
          bt.A = c->taubuf.p + (cc - 1) * tcs + (long)gr[q].ch0 * nz * O * n;
          bt.B = PV + cc * compP;
          RET(gemm(c, bt));
        }
      }
      if (gga) {
        // tag 5 cost of this group's M-backward, whichever kernel runs it.  flops: the
        // PhiO^T M GEMM (2 O per M element) + generating M = sum_c wv_c dPhiV_c (3 FMAs per
        // M element); bytes: PhiO0, dPhiV_{x,y,z}, wv in, accT read + written
        const double m_flops = 2.0 * (O + 3) * (double)nzg * V * n;
        const double m_bytes = 8.0 * ((double)n * O + 3.0 * n * V + 3.0 * n * nzg + 2.0 * O * (double)nzg * V);
        if (O <= 128 && c->m_kernel) {
          // dedicated kernel (xt_xcm.hip); tag 5 timing around it and its reduce
          const size_t need = xc_back_m_workspace_bytes(O, nzg, V, n);
          if (c->ws.n * sizeof(double) < need) RET(c->ws.ensure(need / sizeof(double) + 1));
          RET(profiled(c, 5, m_flops, m_bytes, "xc_back_m", [&] {
            return xc_back_m(O, nzg, V, n, PO, nmo, PV + compP, compP, nmo, Rg[q], ldR[q],
                             c->accT.p + gr[q].ch0 * chs, (long)nzg * V, c->ws.p, c->ws.n * sizeof(double), c->st);
          }));
          continue;
        }
        GemmDesc b2;   // accT[i][(xg,a)] += sum_g PhiO0[g][i] sum_c wv_c[g][xg] dPhiV_c[g][a]
        b2.M = O; b2.N = xc_m_cols(nzg, V, xc_m_bn()); b2.K = n;
        b2.A = PO; b2.sAm = 1; b2.sAk = nmo;
        b2.fz.mode = 2; b2.fz.V = V; b2.fz.nx = nzg; b2.fz.mbn = xc_m_bn();
        b2.fz.w = PV + compP; b2.fz.wc = compP; b2.fz.wg = nmo;
        b2.fz.rho = Rg[q]; b2.fz.rg = ldR[q];
        b2.C = c->accT.p + gr[q].ch0 * chs; b2.ldc = (long)nzg * V; b2.beta = 1.0;
        b2.tag = 5;
        b2.flops = m_flops; b2.bytes = m_bytes;
        RET(gemm(c, b2));
      }
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------
// VV10 (NLC) response over the NLC grid (XTDA.py:515-517), in chunks of G points:
//   forward  Uc = {PhiV0, dPhiV_x, dPhiV_y, dPhiV_z} Ze^T            (4 GEMMs per group, tag 2)
//            rho1, grad rho1 summed over both spin channels, gamma1 = 2 grad rho0 . grad rho1
//   xt_vv10_response over the whole grid: (vrho1, vgamma1)
//   back     L0 = wv0 PhiO + wv . dPhiO, Lc = wv_c PhiO;  acc += L0^T PhiV0 + sum_c Lc^T dPhiV_c
//                                                                     (4 GEMMs per group, tag 3)
// The potential is the same for both spins; each channel projects it onto its own block.
// ---------------------------------------------------------------------------
int xt::nlc_response(xt_ctx* c, int nz) {
  const int O = c->O, V = c->V, nmo = c->d.nmo, ng = c->nlc_ng, nch = c->nchan;
  const long chs = (long)nz * O * V;
  Group gr[2];
  const int ngr = channel_groups(c, gr);
  const size_t per_g = (size_t)4 * nch * nz * O;
  const size_t G = grid_chunk(c, (size_t)4 << 30, per_g, ng);
  RET(c->nlcU.ensure(per_g * G));
  RET(c->nlcR.ensure((size_t)7 * nz * ng));
  double* rho1 = c->nlcR.p;
  double* gam1 = rho1 + (size_t)nz * ng;
  double* grad1 = gam1 + (size_t)nz * ng;
  double* vr1 = grad1 + (size_t)3 * nz * ng;
  double* vg1 = vr1 + (size_t)nz * ng;
  const long compP = (long)ng * nmo;
  const long basP = 4 * compP;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1)
      RET(xt_vv10_response(ng, nlc_xyz(c), nlc_plane(c, NLC_W), nlc_plane(c, NLC_RHO), nlc_plane(c, NLC_GAM),
                           c->nlc_b, c->nlc_C, c->nlc_rho_min, nlc_plane(c, NLC_SUMS), nz, rho1, gam1, 0, ng, vr1,
                           vg1, c->st));
    for (int g0 = 0; g0 < ng; g0 += (int)G) {
      const int n = (g0 + (int)G <= ng) ? (int)G : ng - g0;
      const long tcs = (long)nch * nz * O * n;
      double* Ug[2]; long ldU[2];
      for (int q = 0; q < ngr; ++q) {
        Ug[q] = c->nlcU.p + (long)gr[q].ch0 * nz * O * n;
        ldU[q] = (long)gr[q].nch * nz * O;
      }
      // spin s -> (group, row offset inside the group)
      double* Us[2]; long lus[2]; const double* Ps[2];
      for (int s = 0; s < 2; ++s) {
        const int q = (ngr == 1) ? 0 : s;
        Us[s] = Ug[q] + (long)((ngr == 1) ? s : 0) * nz * O; lus[s] = ldU[q];
        Ps[s] = c->nlcPhi.p + c->occ_basis[s] * basP + (long)g0 * nmo;
      }
      if (pass == 1)
        vv10_back_l(c->st, n, g0, ng, nz, O, nmo, compP, Ps[0], Ps[1], Us[0], lus[0], Us[1], lus[1], tcs,
                    nlc_plane(c, NLC_GRAD), nlc_plane(c, NLC_VG), vr1, vg1, grad1);
      for (int q = 0; q < ngr; ++q) {
        const int nzg = gr[q].nch * nz;
        const double* PV = c->nlcPhi.p + gr[q].vb * basP + (long)g0 * nmo + c->v0;
        for (int cc = 0; cc < 4; ++cc) {
          GemmDesc g;
          if (pass == 0) {   // Ucc[g][(x,i)] = sum_a PVcc[g][a] Ze[(x,i)][a]
            g.M = n; g.N = nzg * O; g.K = V;
            g.A = PV + cc * compP; g.sAm = nmo; g.sAk = 1;
            g.B = c->ze.p + gr[q].ch0 * chs; g.sBn = V; g.sBk = 1;
            g.C = Ug[q] + cc * tcs; g.ldc = ldU[q];
            g.tag = 2;
          } else {           // acc[(x,i)][a] += sum_g Lcc[g][(x,i)] PVcc[g][a]
            g.M = nzg * O; g.N = V; g.K = n;
            g.A = Ug[q] + cc * tcs; g.sAm = 1; g.sAk = ldU[q];
            g.B = PV + cc * compP; g.sBk = nmo; g.sBn = 1;
            g.C = c->acc.p + gr[q].ch0 * chs; g.ldc = V; g.beta = 1.0;
            g.tag = 3;
          }
          RET(gemm(c, g));
        }
      }
      if (pass == 0)
        vv10_forward(c->st, n, g0, ng, nz, O, nmo, compP, Ps[0], Ps[1], Us[0], lus[0], Us[1], lus[1], tcs,
                     nlc_plane(c, NLC_GRAD), rho1, gam1, grad1);
    }
  }
  return 0;
}
