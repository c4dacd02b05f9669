// xt_ctx: the operator context shared by its three translation units (host only).
//   xt_ctx.hip     the context itself: setup, one-electron terms, xt_apply
//   xt_ctx_jk.hip  everything that knows the layout of the MO factor (Bmo) and of the
//                  stored exchange (Kx)
//   xt_ctx_xc.hip  everything that knows the layout of the MO values on the two grids
//                  (Phi, nlcPhi) and of the weighted kernel (kern)
#pragma once
#include <vector>
#include "xt_host.h"

struct xt_ctx {
  xt_desc d;
  hipStream_t st = nullptr;
  int nbasis = 1;            // MO bases: 1 restricted, 2 unrestricted
  int ncomp = 1;                 // MO planes on the grid: value (+ 3 gradients for GGA / MGGA)
  int nkc = 1;                   // kernel components: 1 LDA, 4 GGA, 5 MGGA (+ tau)
  int nchan = 2;             // spin channels in the trial vector
  int O = 0, V = 0, v0 = 0;  // superset occupied / virtual dims, vir MO offset
  int occ_basis[2] = {0, 0}, vir_basis[2] = {0, 0};
  double ck = 0.0, ck_lr = 0.0;
  bool has_orb = false, has_df = false, has_lr = false, has_grid = false, has_fock = false, has_eps = false;
  bool has_vects = false;    // XSF OO basis set (empty for a doublet: no^2 - 1 = 0)
  xt::DevBuf C, Bmo, Bmo_lr, Phi, kern, F, eps, vects;
  xt::DevBuf ze, acc, kx, zr, tbuf, ubuf, gam, gam2, ws, stage, stage2, zin, sout, trace;
  xt::DevBuf zp, accT, wbuf, taubuf;
  hipEvent_t ev[5];
  double timings[4] = {0, 0, 0, 0};
  // live per-kernel timing of tagged GEMM classes (bench roofline); mask bit t = tag t
  int prof_mask = 0;
  std::vector<hipEvent_t> pev;     // pairs
  std::vector<int> pev_tag;
  int pev_used = 0;
  double prof_flops[6] = {0, 0, 0, 0, 0, 0};
  double prof_bytes[6] = {0, 0, 0, 0, 0, 0};   // compulsory HBM bytes (operands once)
  double prof_ms[6] = {0, 0, 0, 0, 0, 0};
  int prof_launches[6] = {0, 0, 0, 0, 0, 0};
  int chol_rank = 0;         // full Cholesky rank of the last xt_set_jk_eri8
  // exchange evaluation (xt_set_exchange_mode): stored MO exchange matrix per channel group
  int kmode = XT_K_AUTO;
  double k_max_bytes = 0.0;  // auto-mode cap (0: free HBM minus a reserve)
  int k_resolved = -1;       // -1 undecided, 0 direct (DF sandwich), 1 stored
  bool kx_valid = false;
  xt::DevBuf Kx;
  // rank partition (xt_set_partition): aux window for J / direct exchange / XSF
  // Delta-A over the resident factor, and the occupied rows of the stored exchange
  int win_p0 = 0, win_np = -1;   // -1: all aux rows
  bool m_kernel = true;          // XC M-backward through xt_xcm.hip (XT_M_KERNEL=0: the engine's mode 2)
  int w_kernel = 2;              // XC rho-forward: 1 xt_xcw.hip, 0 the engine's mode 1, 2 by size (XT_W_KERNEL)
  int kr0 = 0, kr1 = -1;         // -1: all O rows
  bool trimmed = false;          // the MO factor holds only this rank's aux window (xt_prepare)
  int naux_full = 0;             // desc naux before the trim
  size_t chunk_bytes = 0;        // XT_CHUNK_BYTES: cap on every chunk-loop byte budget (0: not set)
  // VV10 non-local correlation (xt_set_nlc): its own grid, MO values on it and the ground-state data
  bool has_nlc = false;
  int nlc_ng = 0;
  double nlc_b = 0.0, nlc_C = 0.0, nlc_rho_min = 0.0;
  xt::DevBuf nlcPhi;             // (nbasis, 4, nlc_ng, nmo)
  xt::DevBuf nlcG;               // per point: xyz (3) | w | rho0 | gamma0 | grad rho0 (3 planes) | sums (6 planes) | dE/dgamma
  xt::DevBuf nlcU, nlcR;         // per apply: the 4 U / L planes of a chunk; rho1, gamma1, grad rho1 (3), vrho1, vgamma1
};

namespace xt {

inline bool is_sf(const xt_desc& d) {
  return d.kind == XT_KIND_SF_DOWN || d.kind == XT_KIND_SF_UP || d.kind == XT_KIND_XSF;
}

// byte budget of a chunked loop: its default, capped by XT_CHUNK_BYTES when that is set
inline size_t chunk_budget(const xt_ctx* c, size_t dflt) {
  return (c->chunk_bytes > 0 && c->chunk_bytes < dflt) ? c->chunk_bytes : dflt;
}

// aux rows this context contracts over (its window of the resident factor)
inline int naux_w(const xt_ctx* c) { return c->win_np < 0 ? c->d.naux : c->win_np; }
// basis block of an MO factor, full rows / from the window start
inline const double* bmo_full(const xt_ctx* c, const DevBuf& B, int basis) {
  return B.p + (size_t)basis * c->d.naux * c->d.nmo * c->d.nmo;
}
inline const double* bmo_of(xt_ctx* c, const DevBuf& B, int basis) {
  return bmo_full(c, B, basis) + (size_t)c->win_p0 * c->d.nmo * c->d.nmo;
}
inline int krow0(const xt_ctx* c) { return c->kr0; }
inline int krow1(const xt_ctx* c) { return c->kr1 < 0 ? c->O : c->kr1; }

// nlcG planes (each nlc_ng doubles; xyz is one block of 3 nlc_ng)
inline double* nlc_xyz(const xt_ctx* c) { return c->nlcG.p; }
inline double* nlc_plane(const xt_ctx* c, int k) { return c->nlcG.p + (size_t)(3 + k) * c->nlc_ng; }
enum { NLC_W = 0, NLC_RHO = 1, NLC_GAM = 2, NLC_GRAD = 3, NLC_SUMS = 6, NLC_VG = 12, NLC_PLANES = 13 };

// ---------------------------------------------------------------------------
// Channel groups.  Spin channels that share one MO basis are contracted
// together (ROKS X-TDA: both channels form one group of 2*nz "vectors"; UKS:
// one group per channel; SF/XSF: one channel).  Per group (channels ch0..ch0+nch-1,
// nzg = nch*nz rows):
//   Ze   : (nzg, O, V) rows of c->ze starting at channel ch0
//   Zp   : (O, nzg, V)  permuted copy for contractions over the occupied index
//   accT : (O, nzg, V)  results of those contractions (exchange, XC back-2),
//          permute-added into acc at the end of xt_apply
// ---------------------------------------------------------------------------
struct Group { int ch0, nch, ob, vb; };
int channel_groups(const xt_ctx* c, Group* g);

// xt_ctx.hip
int to_device(xt_ctx* c, double* dst, const double* src, size_t count, int ptr_kind);   // dst holds count
int to_device(xt_ctx* c, DevBuf& dst, const double* src, size_t count, int ptr_kind);   // dst grown to count
int prof_begin(xt_ctx* c, int tag, double flops, double bytes, bool* on);
int prof_end(xt_ctx* c, int tag, bool on);
int gemm(xt_ctx* c, const GemmDesc& g);
int right_mo(xt_ctx* c, int nz, int nr, int K, int ncl, const double* Z, long ldZ, long svZ, const double* F,
             long sFk, long sFn, double* S, long ldS, long svS, double alpha);
int left_mo(xt_ctx* c, int nz, int nr, int K, int ncl, const double* F, long sFm, long sFk, const double* Z,
            long ldZ, long svZ, double* S, long ldS, long svS, double alpha);
// the three responses of xt_apply, which calls these and none of their parts (xt_ctx_jk.hip, xt_ctx_xc.hip)
int jk_response(xt_ctx* c, int nz);
int xc_response(xt_ctx* c, int nz);
int nlc_response(xt_ctx* c, int nz);

// a dedicated kernel's launch (0 or an error code) under the live timing of its tag
template <class Launch>
int profiled(xt_ctx* c, int tag, double flops, double bytes, const char* name, Launch&& launch) {
  bool prof = false;
  RET(prof_begin(c, tag, flops, bytes, &prof));
  const int r = launch();
  if (r) return fail(r, std::string(name) + " launch failed");
  return prof_end(c, tag, prof);
}

}  // namespace xt
