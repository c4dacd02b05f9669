// xt_tdm_sc: transition moments between spin-conserving roots (X-TDA / U-TDA) and from the
// reference state to them (include/xtddft_amd.h; X_TDA.calculate_TDM, xtddft/XTDA.py:1354-1400,
// over TDM_S / TDM_GSS, x2c_hamiltonian/driver/tdm.py:6-126).
//
// The reference evaluates up to 18 einsum terms per ordered pair of states.  They are bilinear
// in the two states, T_x[L,R] = <z_L, Y_x[R]>, so Y = dT/dz_L is built once per state, in the
// layout of the vector rows themselves ([za | zb], PySCF order), and one Gram product over dim
// gives all pairs:
//
//   d_oo, d_vv per spin and component, d_ov into the packed image [d^a_ov | d^b_ov]   engine GEMMs
//   Y^s[x,R] = Z^s_R d^s_vv[x] - d^s_oo[x] Z^s_R, s = a, b      engine GEMMs on the rows in place
//   spin-adapted, no > 0 (cv1 = (cva - cvb)/sqrt 2 in utils.so2st's phase, h = g - 1/sqrt 2):
//     cv1[R]                                                      k_sc_cv1
//     Ycv1[x,R] = co_R d_ov[x] + d_co[x] ov_R                     engine GEMMs
//     Y_co[x,R] -= h cv1_R d_ov[x]^T,  Y_ov[x,R] -= h d_co[x]^T cv1_R
//     Y_cva -= (h/sqrt 2) Ycv1,  Y_cvb += (h/sqrt 2) Ycv1         k_sc_scatter
//   T[x] = Z Y[x]^T                                               engine GEMM over dim
//   ground row: image (ncomp x dim) times Z^T, mirrored into row and column 0    k_sc_ground
//
// In so2st's phase the couplings of CV(1) with CO(0) and OV(0) carry -g, g = sqrt((S+1)/(2S));
// tdm.py:116-125 writes +g for a CV(1) of the opposite sign.  With g = 1/sqrt 2 (h = 0) the
// spin-orbital formula is recovered.
//
// States are processed in chunks so that what grows with nstates stays within a budget; every
// product has a shape that depends only on the descriptor and the chunk size, so the split-K
// plans and with them the bits repeat.  No atomics anywhere.
#include <hip/hip_runtime.h>
#include <math.h>
#include "xt_host.h"

using namespace xt;

namespace {

#define GRID_STRIDE(i, n) \
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

inline int nblocks(long n, int cap = 2048) {   // bandwidth-bound passes: capped grid, strided
  long b = (n + 255) / 256;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

// cv1[s,i,a] = (za[s,i,a] - zb[s,i,no+a]) / sqrt 2 for the core rows i < nc; ns states of
// dim doubles, za at 0 (row pitch nv), zb at na (row pitch no + nv)
__global__ void k_sc_cv1(long ns, int nc, int no, int nv, long dim, long na, const double* __restrict__ z,
                         double* __restrict__ cv1) {
  const long cv = (long)nc * nv;
  GRID_STRIDE(t, ns * cv) {
    const long s = t / cv, k = t % cv;
    const int i = (int)(k / nv), a = (int)(k % nv);
    const double* zs = z + s * dim;
    cv1[t] = (zs[k] - zs[na + (long)i * (no + nv) + no + a]) * M_SQRT1_2;
  }
}

// y_cva[x,s,i,a] += f ycv1[x,s,i,a], y_cvb[x,s,i,a] -= f ycv1[x,s,i,a]; nxs = ncomp * ns rows
__global__ void k_sc_scatter(long nxs, int nc, int no, int nv, long dim, long na, double f,
                             const double* __restrict__ ycv1, double* __restrict__ y) {
  const long cv = (long)nc * nv;
  GRID_STRIDE(t, nxs * cv) {
    const long r = t / cv, k = t % cv;
    const int i = (int)(k / nv), a = (int)(k % nv);
    double* ys = y + r * dim;
    const double v = f * ycv1[t];
    ys[k] += v;
    ys[na + (long)i * (no + nv) + no + a] -= v;
  }
}

// out (ncomp, n1, n1), n1 = nstates + 1: out[x,0,0] = 0, out[x,0,1+s] = out[x,1+s,0] = g[x,s]
__global__ void k_sc_ground(int ncomp, int nstates, const double* __restrict__ g, double* __restrict__ out) {
  const long n1 = nstates + 1;
  GRID_STRIDE(t, (long)ncomp * n1) {
    const long x = t / n1, s = t % n1;
    double* o = out + x * n1 * n1;
    if (s == 0) { o[0] = 0.0; continue; }
    const double v = g[x * nstates + s - 1];
    o[s] = v;
    o[s * n1] = v;
  }
}

const char* const what = "xt_tdm_sc";   // message prefix

}  // namespace

extern "C" int xt_tdm_sc(const xt_tdm_sc_desc* desc, const double* op_ao, const double* c_occ_a,
                         const double* c_vir_a, const double* c_occ_b, const double* c_vir_b, const double* vecs,
                         double* out, int ptr_kind, void* stream) {
  // ---- validation: before any HIP call ----
  if (!desc) return set_error(XT_ERR_ARG, "xt_tdm_sc: null descriptor");
  const xt_tdm_sc_desc d = *desc;
  if (d.nao < 1) return set_error(XT_ERR_ARG, "xt_tdm_sc: nao < 1");
  if (d.ncomp < 1) return set_error(XT_ERR_ARG, "xt_tdm_sc: ncomp < 1");
  if (d.nstates < 1) return set_error(XT_ERR_ARG, "xt_tdm_sc: nstates < 1");
  if (d.nocc_a < 0 || d.nvir_a < 0 || d.nocc_b < 0 || d.nvir_b < 0 ||
      (long)d.nocc_a * d.nvir_a + (long)d.nocc_b * d.nvir_b < 1)
    return set_error(XT_ERR_ARG, "xt_tdm_sc: bad orbital counts (need blocks >= 0 and dim >= 1)");
  if ((long)d.nocc_a * d.nvir_a + (long)d.nocc_b * d.nvir_b >= (1L << 21))   // the engine's 32-bit tile offsets
    return set_error(XT_ERR_ARG, "xt_tdm_sc: dim >= 2^21 is beyond the GEMM engine's row pitch");
  if (d.spin_adapted != 0 && d.spin_adapted != 1) return set_error(XT_ERR_ARG, "xt_tdm_sc: spin_adapted must be 0 or 1");
  if (d.spin_adapted && (d.no < 0 || d.nocc_a - d.nocc_b != d.no || d.nvir_b - d.nvir_a != d.no))
    return set_error(XT_ERR_ARG, "xt_tdm_sc: inconsistent ROKS counts (need nocc_a - nocc_b = nvir_b - nvir_a = no >= 0)");
  if (d.spin_adapted && d.no > 0 && !(d.si > 0.0))
    return set_error(XT_ERR_ARG, "xt_tdm_sc: spin adaptation with open shells needs S > 0");
  if (d.with_ground != 0 && d.with_ground != 1) return set_error(XT_ERR_ARG, "xt_tdm_sc: with_ground must be 0 or 1");
  if (!op_ao || !vecs || !out || (d.nocc_a > 0 && !c_occ_a) || (d.nvir_a > 0 && !c_vir_a) ||
      (d.nocc_b > 0 && !c_occ_b) || (d.nvir_b > 0 && !c_vir_b))
    return set_error(XT_ERR_ARG, "xt_tdm_sc: null argument");
  if (ptr_kind != XT_PTR_HOST && ptr_kind != XT_PTR_DEVICE) return set_error(XT_ERR_ARG, "xt_tdm_sc: bad ptr_kind");

  hipStream_t st = (hipStream_t)stream;
  const bool host = ptr_kind == XT_PTR_HOST;
  const int nao = d.nao, X = d.ncomp, N = d.nstates, G = d.with_ground;
  const int Oa = d.nocc_a, Va = d.nvir_a, Ob = d.nocc_b, Vb = d.nvir_b;
  const long na = (long)Oa * Va, nb = (long)Ob * Vb, dim = na + nb;
  const long N1 = N + G;
  // the correction couples the core rows of za with the [o|v] columns of zb
  const int no = d.no, nc = Ob, nv = Va;
  const bool corr = d.spin_adapted && no > 0 && nc > 0 && nv > 0;
  const long cv = corr ? (long)nc * nv : 0;
  const double h = corr ? sqrt((d.si + 1.0) / (2.0 * d.si)) - M_SQRT1_2 : 0.0;

  // states per chunk: Y for every component, the two uploaded chunks, cv1 and Ycv1 within
  // the budget (tdm_budget_mib)
  const double per_state = 8.0 * ((double)(X + 2) * dim + (double)(X + 1) * cv);
  long ns = (long)(tdm_budget_mib() * 1048576.0 / per_state);
  if (ns > 32768 / X) ns = 32768 / X;   // (state, component) batches of one launch: grid z
  ns = ns < 1 ? 1 : (ns > N ? N : ns);
  if ((long)X * ns > 32768) return set_error(XT_ERR_ARG, "xt_tdm_sc: ncomp > 32768");

  // ---- inputs on the device ----
  TmpBuf b_op, b_coa, b_cva, b_cob, b_cvb, b_out;
  RET(upload(b_op, op_ao, (size_t)X * nao * nao, ptr_kind, st, what));
  RET(upload(b_coa, c_occ_a, (size_t)nao * Oa, ptr_kind, st, what));
  RET(upload(b_cva, c_vir_a, (size_t)nao * Va, ptr_kind, st, what));
  RET(upload(b_cob, c_occ_b, (size_t)nao * Ob, ptr_kind, st, what));
  RET(upload(b_cvb, c_vir_b, (size_t)nao * Vb, ptr_kind, st, what));
  double* outd = out;
  if (host) { RET(b_out.ensure((size_t)X * N1 * N1, what)); outd = b_out.p; }

  // ---- engine launches (split-K workspace grown on demand, 256 MiB cap) ----
  TmpBuf ws;
  auto run = [&](const GemmDesc& g) -> int {
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || g.nb1 <= 0 || g.nb2 <= 0) return 0;   // empty block: nothing is launched
    return run_gemm(g, st, ws, (size_t)256 << 20, 0, what, "GEMM launch failed");
  };

  // ---- d_oo, d_vv per spin and component; d_ov straight into the ground image ----
  const int oab = Oa > Ob ? Oa : Ob, vab = Va > Vb ? Va : Vb;
  TmpBuf b_half, b_doa, b_dva, b_dob, b_dvb, b_img, b_g;
  RET(b_half.ensure((size_t)X * nao * (oab > vab ? oab : vab), what));
  RET(b_doa.ensure((size_t)X * Oa * Oa, what));
  RET(b_dva.ensure((size_t)X * Va * Va, what));
  RET(b_dob.ensure((size_t)X * Ob * Ob, what));
  RET(b_dvb.ensure((size_t)X * Vb * Vb, what));
  if (G) { RET(b_img.ensure((size_t)X * dim, what)); RET(b_g.ensure((size_t)X * N, what)); }
  auto half = [&](const double* cm, int n) -> int {   // half[x] = op[x] C
    GemmDesc g;
    g.M = nao; g.N = n; g.K = nao; g.nb1 = X;
    g.A = op_ao; g.sAm = nao; g.sAk = 1; g.sAb1 = (long)nao * nao;
    g.B = cm; g.sBk = n; g.sBn = 1;
    g.C = b_half.p; g.ldc = n; g.sCb1 = (long)nao * n;
    return run(g);
  };
  auto project = [&](const double* cl, int nl, int nr, double* dst, long sdst) -> int {   // dst[x] = Cl^T half[x]
    GemmDesc g;
    g.M = nl; g.N = nr; g.K = nao; g.nb1 = X;
    g.A = cl; g.sAm = 1; g.sAk = nl;
    g.B = b_half.p; g.sBk = nr; g.sBn = 1; g.sBb1 = (long)nao * nr;
    g.C = dst; g.ldc = nr; g.sCb1 = sdst;
    return run(g);
  };
  auto spin_blocks = [&](const double* co, const double* cvr, int O, int V, double* doo, double* dvv, long off) -> int {
    if (O <= 0 || V <= 0) return 0;   // an empty amplitude block needs no operator
    RET(half(co, O));
    RET(project(co, O, O, doo, (long)O * O));
    RET(half(cvr, V));
    RET(project(cvr, V, V, dvv, (long)V * V));
    if (G) RET(project(co, O, V, b_img.p + off, dim));
    return 0;
  };
  RET(spin_blocks(c_occ_a, c_vir_a, Oa, Va, b_doa.p, b_dva.p, 0));
  RET(spin_blocks(c_occ_b, c_vir_b, Ob, Vb, b_dob.p, b_dvb.p, na));

  // ---- state chunks ----
  TmpBuf b_zj, b_zi, b_y, b_cv1, b_ycv1;
  if (host) RET(b_zj.ensure((size_t)ns * dim, what));
  if (host && ns < N) RET(b_zi.ensure((size_t)ns * dim, what));
  RET(b_y.ensure((size_t)X * ns * dim, what));
  if (corr) { RET(b_cv1.ensure((size_t)ns * cv, what)); RET(b_ycv1.ensure((size_t)X * ns * cv, what)); }
  auto load_chunk = [&](long s0, long n, double* buf, const double** z) -> int {
    const double* src = vecs + s0 * dim;
    if (host) {
      HIPCHK(what, hipMemcpyAsync(buf, src, (size_t)n * dim * 8, hipMemcpyHostToDevice, st));
      src = buf;
    }
    *z = src;
    return 0;
  };
  // Y^s[x,R] = Z^s_R d_vv[x] - d_oo[x] Z^s_R on the block at `off` of every row
  auto channel = [&](const double* zj, long nj, int O, int V, const double* doo, const double* dvv, long off) -> int {
    GemmDesc g;
    g.M = O; g.N = V; g.K = V; g.nb1 = (int)nj; g.nb2 = X;
    g.A = zj + off; g.sAm = V; g.sAk = 1; g.sAb1 = dim;
    g.B = dvv; g.sBk = V; g.sBn = 1; g.sBb2 = (long)V * V;
    g.C = b_y.p + off; g.ldc = V; g.sCb1 = dim; g.sCb2 = nj * dim;
    RET(run(g));
    GemmDesc q;
    q.M = O; q.N = V; q.K = O; q.nb1 = (int)nj; q.nb2 = X;
    q.A = doo; q.sAm = O; q.sAk = 1; q.sAb2 = (long)O * O;
    q.B = zj + off; q.sBk = V; q.sBn = 1; q.sBb1 = dim;
    q.C = b_y.p + off; q.ldc = V; q.sCb1 = dim; q.sCb2 = nj * dim;
    q.alpha = -1.0; q.beta = 1.0;
    return run(q);
  };

  for (long j0 = 0; j0 < N; j0 += ns) {
    const long nj = N - j0 < ns ? N - j0 : ns;
    const double* zj = nullptr;
    RET(load_chunk(j0, nj, b_zj.p, &zj));
    double* y = b_y.p;
    const long sy = nj * dim;   // component stride of Y
    RET(channel(zj, nj, Oa, Va, b_doa.p, b_dva.p, 0));
    RET(channel(zj, nj, Ob, Vb, b_dob.p, b_dvb.p, na));
    if (corr) {
      // d_ov[x] (no x nv) = d^b_vv[x][o, v]; d_co[x] (nc x no) = d^a_oo[x][c, o]
      const double* dov = b_dvb.p + no;
      const double* dco = b_doa.p + nc;
      const long co_off = na, ov_off = (long)nc * nv;   // co = zb[:, :no], ov = za[nc:, :]
      hipLaunchKernelGGL(k_sc_cv1, dim3(nblocks(nj * cv)), dim3(256), 0, st, nj, nc, no, nv, dim, na, zj, b_cv1.p);
      GemmDesc g;   // Ycv1[x,R] = co_R d_ov[x]
      g.M = nc; g.N = nv; g.K = no; g.nb1 = (int)nj; g.nb2 = X;
      g.A = zj + co_off; g.sAm = Vb; g.sAk = 1; g.sAb1 = dim;
      g.B = dov; g.sBk = Vb; g.sBn = 1; g.sBb2 = (long)Vb * Vb;
      g.C = b_ycv1.p; g.ldc = nv; g.sCb1 = cv; g.sCb2 = nj * cv;
      RET(run(g));
      GemmDesc q;   // Ycv1[x,R] += d_co[x] ov_R
      q.M = nc; q.N = nv; q.K = no; q.nb1 = (int)nj; q.nb2 = X;
      q.A = dco; q.sAm = Oa; q.sAk = 1; q.sAb2 = (long)Oa * Oa;
      q.B = zj + ov_off; q.sBk = nv; q.sBn = 1; q.sBb1 = dim;
      q.C = b_ycv1.p; q.ldc = nv; q.sCb1 = cv; q.sCb2 = nj * cv;
      q.beta = 1.0;
      RET(run(q));
      GemmDesc u;   // Y_co[x,R] -= h cv1_R d_ov[x]^T
      u.M = nc; u.N = no; u.K = nv; u.nb1 = (int)nj; u.nb2 = X;
      u.A = b_cv1.p; u.sAm = nv; u.sAk = 1; u.sAb1 = cv;
      u.B = dov; u.sBk = 1; u.sBn = Vb; u.sBb2 = (long)Vb * Vb;
      u.C = y + co_off; u.ldc = Vb; u.sCb1 = dim; u.sCb2 = sy;
      u.alpha = -h; u.beta = 1.0;
      RET(run(u));
      GemmDesc w;   // Y_ov[x,R] -= h d_co[x]^T cv1_R
      w.M = no; w.N = nv; w.K = nc; w.nb1 = (int)nj; w.nb2 = X;
      w.A = dco; w.sAm = 1; w.sAk = Oa; w.sAb2 = (long)Oa * Oa;
      w.B = b_cv1.p; w.sBk = nv; w.sBn = 1; w.sBb1 = cv;
      w.C = y + ov_off; w.ldc = nv; w.sCb1 = dim; w.sCb2 = sy;
      w.alpha = -h; w.beta = 1.0;
      RET(run(w));
      // the component-major Y rows (x, R) and Ycv1 rows (x, R) pair up one to one
      hipLaunchKernelGGL(k_sc_scatter, dim3(nblocks((long)X * nj * cv)), dim3(256), 0, st, (long)X * nj, nc, no, nv,
                         dim, na, -h * M_SQRT1_2, b_ycv1.p, y);
    }
    if (G) {
      GemmDesc g;   // g[x, R] = <image[x], z_R>
      g.M = X; g.N = (int)nj; g.K = (int)dim;
      g.A = b_img.p; g.sAm = dim; g.sAk = 1;
      g.B = zj; g.sBk = 1; g.sBn = dim;
      g.C = b_g.p + j0; g.ldc = N;
      RET(run(g));
    }
    for (long i0 = 0; i0 < N; i0 += ns) {
      const long ni = N - i0 < ns ? N - i0 : ns;
      const double* zi = zj;
      if (i0 != j0) RET(load_chunk(i0, ni, b_zi.p, &zi));
      GemmDesc g;   // T[x, L, R] = <z_L, Y[x, R]>
      g.M = (int)ni; g.N = (int)nj; g.K = (int)dim; g.nb1 = X;
      g.A = zi; g.sAm = dim; g.sAk = 1;
      g.B = y; g.sBk = 1; g.sBn = dim; g.sBb1 = sy;
      g.C = outd + (i0 + G) * N1 + (j0 + G); g.ldc = N1; g.sCb1 = N1 * N1;
      RET(run(g));
    }
  }
  if (G)
    hipLaunchKernelGGL(k_sc_ground, dim3(nblocks((long)X * N1)), dim3(256), 0, st, X, N, b_g.p, outd);
  HIPCHK(what, hipGetLastError());
  if (host) HIPCHK(what, hipMemcpyAsync(out, outd, (size_t)X * N1 * N1 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(what, hipStreamSynchronize(st));   // the workspace is released on return
  return 0;
}
