// xt_si_couple: the bilinear couplings of a one-electron MO operator between the states of the
// three TDA manifolds and the reference state (include/xtddft_amd.h; SI_driver.make_hso_local /
// make_dm_local, x2c_hamiltonian/driver/si_driver.py:472-916, over the tables of
// x2c_hamiltonian/driver/tdm.py:128-238).
//
// The reference evaluates up to 24 einsum terms with explicit delta matrices per ordered pair
// of states.  Every term is linear in the operator with a real factor that depends on S only,
// and bilinear in the two states: T_x[L,R] = <z_L, Y_x[R]>.  Y is the operator's image of the
// right-hand states in the LEFT manifold's layout, so per pair of groups
//
//   Y[x,R] block by block: every term is f M X (left) or f X M (right) with M a block of
//   D[x] over [c|o|v], plain or transposed -- addressed in place by its strides, so the
//   antisymmetric operator needs no copy and no sign table                    engine GEMMs
//   the O1O1 vector of |S->: its (a + b delta) images into CO / OV / O1O2       k_si_o_spread
//   and the O1O1 rows of Y, fixed-order sums over c, o and v                    k_si_o_gather
//   T[x] = Z_L Y[x]^T, one rectangular product over the left layout's dim       engine GEMM
//   reference-state rows / column: images of D's blocks (k_si_image) times Z^T, placed by
//   k_si_place
//
// Group order |S->, |GS>, |So>, |S+> (the reference's H_eff).  XT_SI_SOC fills the square
// same-manifold blocks and the blocks with L before R; XT_SI_DIPOLE the same-S blocks.  All
// else stays zero.
//
// States are processed in chunks so that what grows with the number of states stays within a
// budget; every product has a shape that depends only on the descriptor and the chunk size, so
// the split-K plans and with them the bits repeat.  No atomics anywhere.
#include <hip/hip_runtime.h>
#include <math.h>
#include <vector>
#include "xt_host.h"

using namespace xt;

namespace {

#define GRID_STRIDE(i, n) \
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

inline int nblocks(long n, int cap = 2048) {   // bandwidth-bound passes: capped grid, strided
  long b = (n + 255) / 256;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

// img[x, r, c] = f D[x][r sr + c sc] for an (rows x cols) block; d already points at the
// block's origin in D[0], img at the block's place in row x = 0 (row pitch dim)
__global__ void k_si_image(int ncomp, int rows, int cols, long sr, long sc, long nmo2, double f,
                           const double* __restrict__ d, double* __restrict__ img, long dim) {
  const long rc = (long)rows * cols;
  GRID_STRIDE(t, (long)ncomp * rc) {
    const long x = t / rc, k = t % rc;
    const long r = k / cols, c = k % cols;
    img[x * dim + k] = f * d[x * nmo2 + r * sr + c * sc];
  }
}

// out[x sx + s ss] = g[x ldg + s], s < cnt
__global__ void k_si_place(int ncomp, long cnt, const double* __restrict__ g, long ldg, double* __restrict__ out,
                           long sx, long ss) {
  GRID_STRIDE(t, (long)ncomp * cnt) {
    const long x = t / cnt, s = t % cnt;
    out[x * sx + s * ss] = g[x * ldg + s];
  }
}

// factors of the O1O1 vector w (length no, sum sw) of a right-hand |S-> state:
//   Y_co[i,u] += D_oc[u,i] (a1 sw + b1 w[u]);  Y_ov[u,a] += D_vo[a,u] (a2 sw + b2 w[u]);
//   Y_oo[v,u] += D_oo[u,v] (cu w[u] + cv w[v] + cs sw)
struct OSpread { double a1, b1, a2, b2, cu, cv, cs; };

// ns right-hand states of dimr doubles (O1O1 at o4), Y rows (x, s) of diml doubles with CO,
// OV, O1O2 at y1, y2, y3
__global__ void k_si_o_spread(int ncomp, long ns, int nc, int no, int nv, OSpread p, const double* __restrict__ d,
                              const double* __restrict__ z, long dimr, long o4, double* __restrict__ y, long diml,
                              long y1, long y2, long y3) {
  const long nmo = nc + no + nv, co = (long)nc * no, ov = (long)no * nv, per = co + ov + (long)no * no;
  GRID_STRIDE(t, (long)ncomp * ns * per) {
    const long xr = t / per;
    long k = t % per;
    const long x = xr / ns, s = xr % ns;
    const double* w = z + s * dimr + o4;
    const double* dx = d + x * nmo * nmo;
    double* ys = y + xr * diml;
    double sw = 0.0;
    for (int u = 0; u < no; ++u) sw += w[u];
    if (k < co) {
      const long i = k / no, u = k % no;
      ys[y1 + k] += dx[(nc + u) * nmo + i] * (p.a1 * sw + p.b1 * w[u]);
    } else if (k < co + ov) {
      k -= co;
      const long u = k / nv, a = k % nv;
      ys[y2 + k] += dx[(nc + no + a) * nmo + nc + u] * (p.a2 * sw + p.b2 * w[u]);
    } else {
      k -= co + ov;
      const long v = k / no, u = k % no;
      ys[y3 + k] += dx[(nc + u) * nmo + nc + v] * (p.cu * w[u] + p.cv * w[v] + p.cs * sw);
    }
  }
}

// the O1O1 rows of Y from the CO, OV and O1O2 blocks of the right-hand states:
//   q1[u] = sum_i co[i,u] D[m1 + u m1u + i m1i],  q2[u] = sum_a ov[u,a] D[m2 + u m2u + a m2a],
//   r1[t] = sum_v oo[v,t] D_oo[t,v],  r2[t] = sum_u oo[t,u] D_oo[u,t],  ra = sum_t r1[t]
//   Y4[t] = e1b q1[t] + e1a sum q1 + e2b q2[t] + e2a sum q2 + d1 r1[t] + d2 r2[t] + ds ra
struct OGather {
  double e1b, e1a, e2b, e2a, d1, d2, ds;
  long m1, m1u, m1i, m2, m2u, m2a;
  int oo;   // the right-hand layout has an O1O2 block at r3
};

__global__ void k_si_o_gather(int ncomp, long ns, int nc, int no, int nv, OGather p, const double* __restrict__ d,
                              const double* __restrict__ z, long dimr, long r1o, long r2o, long r3o,
                              double* __restrict__ y, long diml, long y4) {
  const long nmo = nc + no + nv;
  GRID_STRIDE(idx, (long)ncomp * ns * no) {
    const long xr = idx / no, t = idx % no;
    const long x = xr / ns, s = xr % ns;
    const double* zs = z + s * dimr;
    const double* dx = d + x * nmo * nmo;
    double q1t = 0.0, q2t = 0.0, s1 = 0.0, s2 = 0.0, r1 = 0.0, r2 = 0.0, ra = 0.0;
    for (int u = 0; u < no; ++u) {
      double q1 = 0.0, q2 = 0.0;
      for (int i = 0; i < nc; ++i) q1 += zs[r1o + (long)i * no + u] * dx[p.m1 + u * p.m1u + i * p.m1i];
      for (int a = 0; a < nv; ++a) q2 += zs[r2o + (long)u * nv + a] * dx[p.m2 + u * p.m2u + a * p.m2a];
      s1 += q1; s2 += q2;
      if (u == t) { q1t = q1; q2t = q2; }
    }
    if (p.oo) {
      const double* oo = zs + r3o;
      for (int v = 0; v < no; ++v) r1 += oo[(long)v * no + t] * dx[(nc + t) * nmo + nc + v];
      for (int u = 0; u < no; ++u) r2 += oo[t * no + u] * dx[(nc + u) * nmo + nc + t];
      for (int u = 0; u < no; ++u) {
        double r = 0.0;
        for (int v = 0; v < no; ++v) r += oo[(long)v * no + u] * dx[(nc + u) * nmo + nc + v];
        ra += r;
      }
    }
    y[xr * diml + y4 + t] = p.e1b * q1t + p.e1a * s1 + p.e2b * q2t + p.e2a * s2 + p.d1 * r1 + p.d2 * r2 + p.ds * ra;
  }
}

const char* const what = "xt_si_couple";   // message prefix

// a block of a state vector: rows x cols of the orbital classes rk, ck (0 c, 1 o, 2 v) at off
struct Blk { long off; int rk, ck; };
struct Layout { long dim = 0; int nb = 0; Blk b[4]; long o4 = 0; };
// Y_dst += f M X_src (side 0) or f X_src M (side 1); tr: M is the transposed block of D
struct Term { int dst, src, side, tr; double f; };
// a block of a reference-state image: img_blk = f D_(rk,ck), or f D_(ck,rk)^T with tr
struct Img { int blk, tr; double f; };

}  // namespace

extern "C" int xt_si_couple(const xt_si_desc* desc, const double* op_mo, const double* x_sm, const double* x_so,
                            const double* x_sp, double* out, int ptr_kind, void* stream) {
  // ---- validation: before any HIP call ----
  if (!desc) return set_error(XT_ERR_ARG, "xt_si_couple: null descriptor");
  const xt_si_desc d = *desc;
  if (d.nc < 0 || d.no < 0 || d.nv < 0 || (long)d.nc + d.no + d.nv < 1)
    return set_error(XT_ERR_ARG, "xt_si_couple: bad orbital counts (need nc, no, nv >= 0 and nmo >= 1)");
  if ((long)d.nc + d.no + d.nv >= (1L << 21))
    return set_error(XT_ERR_ARG, "xt_si_couple: nmo >= 2^21 is beyond the GEMM engine's row pitch");
  if (d.ncomp < 1 || d.ncomp > 32768) return set_error(XT_ERR_ARG, "xt_si_couple: ncomp outside 1..32768");
  if (d.mode != XT_SI_SOC && d.mode != XT_SI_DIPOLE) return set_error(XT_ERR_ARG, "xt_si_couple: bad mode");
  if (d.with_ground != 0 && d.with_ground != 1) return set_error(XT_ERR_ARG, "xt_si_couple: with_ground must be 0 or 1");
  if (d.n_sm < 0 || d.n_so < 0 || d.n_sp < 0 || (long)d.n_sm + d.n_so + d.n_sp + d.with_ground < 1)
    return set_error(XT_ERR_ARG, "xt_si_couple: bad state counts (need n_sm, n_so, n_sp >= 0 and one state at least)");
  if ((long)d.n_sm + d.n_so + d.n_sp + d.with_ground > 46340)
    return set_error(XT_ERR_ARG, "xt_si_couple: more than 46340 states");
  if (!(d.s >= 0.0) || fabs(2.0 * d.s - d.no) > 1e-9)
    return set_error(XT_ERR_ARG, "xt_si_couple: s must equal no / 2 (the high-spin reference)");
  if (d.n_sm > 0 && d.s < 1.0 - 1e-9) return set_error(XT_ERR_ARG, "xt_si_couple: |S-> states need S >= 1");
  const long cv = (long)d.nc * d.nv, co = (long)d.nc * d.no, ov = (long)d.no * d.nv, oo = (long)d.no * d.no;
  const long dim_sm = cv + co + ov + oo + d.no, dim_so = cv + co + ov + cv, dim_sp = cv;
  if (dim_sm >= (1L << 21) || dim_so >= (1L << 21))   // the engine's 32-bit tile offsets
    return set_error(XT_ERR_ARG, "xt_si_couple: dim >= 2^21 is beyond the GEMM engine's row pitch");
  if ((d.n_sm > 0 && dim_sm < 1) || (d.n_so > 0 && dim_so < 1) || (d.n_sp > 0 && dim_sp < 1))
    return set_error(XT_ERR_ARG, "xt_si_couple: states of an empty manifold (dim 0)");
  if (!op_mo || !out || (d.n_sm > 0 && !x_sm) || (d.n_so > 0 && !x_so) || (d.n_sp > 0 && !x_sp))
    return set_error(XT_ERR_ARG, "xt_si_couple: null argument");
  if (ptr_kind != XT_PTR_HOST && ptr_kind != XT_PTR_DEVICE) return set_error(XT_ERR_ARG, "xt_si_couple: bad ptr_kind");

  hipStream_t st = (hipStream_t)stream;
  const bool host = ptr_kind == XT_PTR_HOST;
  const int nc = d.nc, no = d.no, nv = d.nv, X = d.ncomp, G = d.with_ground;
  const long nmo = (long)nc + no + nv, nmo2 = nmo * nmo;
  const double S = d.s;
  const bool soc = d.mode == XT_SI_SOC, open = S > 1e-9;
  // groups 0 |S->, 1 |GS>, 2 |So>, 3 |S+>: counts, first row of the result, vectors, layouts
  const long cnt[4] = {d.n_sm, G, d.n_so, d.n_sp};
  const long first[4] = {0, cnt[0], cnt[0] + cnt[1], cnt[0] + cnt[1] + cnt[2]};
  const long n = first[3] + cnt[3];
  const double* vec[4] = {x_sm, nullptr, x_so, x_sp};
  Layout lay[4];
  lay[0].dim = dim_sm; lay[0].nb = 4; lay[0].o4 = cv + co + ov + oo;
  lay[0].b[0] = {0, 0, 2}; lay[0].b[1] = {cv, 0, 1}; lay[0].b[2] = {cv + co, 1, 2}; lay[0].b[3] = {cv + co + ov, 1, 1};
  lay[2].dim = dim_so; lay[2].nb = 4;
  lay[2].b[0] = {0, 0, 2}; lay[2].b[1] = {cv, 0, 1}; lay[2].b[2] = {cv + co, 1, 2}; lay[2].b[3] = {cv + co + ov, 0, 2};
  lay[3].dim = dim_sp; lay[3].nb = 1;
  lay[3].b[0] = {0, 0, 2};
  const int kn[3] = {nc, no, nv};            // size of an orbital class
  const long k0[3] = {0, nc, (long)nc + no};   // its first orbital

  // states per chunk: Y for every component and the two uploaded chunks within the budget
  const long dmax = dim_sm > dim_so ? dim_sm : dim_so;
  long ns = (long)(tdm_budget_mib() * 1048576.0 / (8.0 * (double)(X + 2) * (double)(dmax > 0 ? dmax : 1)));
  if (ns > 32768 / X) ns = 32768 / X;   // (state, component) batches of one launch: grid z
  long most = d.n_sm > d.n_so ? d.n_sm : d.n_so;   // the largest group
  if (d.n_sp > most) most = d.n_sp;
  if (ns > most) ns = most;
  if (ns < 1) ns = 1;

  // ---- inputs on the device ----
  TmpBuf b_op, b_out, b_zj, b_zi, b_y, b_img, b_g, ws;
  RET(upload(b_op, op_mo, (size_t)X * nmo2, ptr_kind, st, what));
  double* outd = out;
  if (host) { RET(b_out.ensure((size_t)X * n * n, what)); outd = b_out.p; }
  HIPCHK(what, hipMemsetAsync(outd, 0, (size_t)X * n * n * 8, st));

  auto run = [&](const GemmDesc& g) -> int {
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || g.nb1 <= 0 || g.nb2 <= 0) return 0;   // empty block: nothing is launched
    return run_gemm(g, st, ws, (size_t)256 << 20, 0, what, "GEMM launch failed");
  };
  auto load_chunk = [&](int grp, long s0, long cntc, TmpBuf& buf, const double** z) -> int {
    const double* src = vec[grp] + s0 * lay[grp].dim;
    if (host) {
      RET(buf.ensure((size_t)ns * dmax, what));
      HIPCHK(what, hipMemcpyAsync(buf.p, src, (size_t)cntc * lay[grp].dim * 8, hipMemcpyHostToDevice, st));
      src = buf.p;
    }
    *z = src;
    return 0;
  };
  // M = D_(p,q) (plain) or D_(q,p)^T: origin and the strides of M's rows and columns
  auto opblock = [&](int p, int q, int tr, const double** m, long* sr, long* sc) {
    if (!tr) { *m = op_mo + k0[p] * nmo + k0[q]; *sr = nmo; *sc = 1; }
    else { *m = op_mo + k0[q] * nmo + k0[p]; *sr = 1; *sc = nmo; }
  };

  // ---- one pair of groups with states on both sides ----
  auto couple = [&](int gl, int gr, const std::vector<Term>& terms, const OSpread* sp, const OGather* ga) -> int {
    const long nl = cnt[gl], nr = cnt[gr];
    if (nl < 1 || nr < 1) return 0;
    const Layout &ll = lay[gl], &lr = lay[gr];
    const long diml = ll.dim, dimr = lr.dim;
    const long cs = ns < nr ? ns : nr;
    RET(b_y.ensure((size_t)X * cs * diml, what));
    for (long j0 = 0; j0 < nr; j0 += ns) {
      const long nj = nr - j0 < ns ? nr - j0 : ns;
      const double* zj = nullptr;
      RET(load_chunk(gr, j0, nj, b_zj, &zj));
      double* y = b_y.p;
      const long sy = nj * diml;   // component stride of Y
      HIPCHK(what, hipMemsetAsync(y, 0, (size_t)X * sy * 8, st));
      for (const Term& t : terms) {
        if (t.f == 0.0) continue;
        const Blk &bd = ll.b[t.dst], &bs = lr.b[t.src];
        const int rd = kn[bd.rk], cd = kn[bd.ck], rs = kn[bs.rk], cq = kn[bs.ck];
        const double* m; long sr, sc;
        GemmDesc g;
        g.nb1 = (int)nj; g.nb2 = X;
        g.C = y + bd.off; g.ldc = cd; g.sCb1 = diml; g.sCb2 = sy;
        g.alpha = t.f; g.beta = 1.0;
        if (t.side == 0) {   // (rd x rs) M times (rs x cd) X
          opblock(bd.rk, bs.rk, t.tr, &m, &sr, &sc);
          g.M = rd; g.N = cd; g.K = rs;
          g.A = m; g.sAm = sr; g.sAk = sc; g.sAb2 = nmo2;
          g.B = zj + bs.off; g.sBk = cq; g.sBn = 1; g.sBb1 = dimr;
        } else {             // (rd x cq) X times (cq x cd) M
          opblock(bs.ck, bd.ck, t.tr, &m, &sr, &sc);
          g.M = rd; g.N = cd; g.K = cq;
          g.A = zj + bs.off; g.sAm = cq; g.sAk = 1; g.sAb1 = dimr;
          g.B = m; g.sBk = sr; g.sBn = sc; g.sBb2 = nmo2;
        }
        RET(run(g));
      }
      if (sp && no > 0)
        hipLaunchKernelGGL(k_si_o_spread, dim3(nblocks((long)X * nj * (co + ov + oo))), dim3(256), 0, st, X, nj, nc, no,
                           nv, *sp, op_mo, zj, dimr, lr.o4, y, diml, ll.b[1].off, ll.b[2].off, ll.b[3].off);
      if (ga && no > 0)
        hipLaunchKernelGGL(k_si_o_gather, dim3(nblocks((long)X * nj * no)), dim3(256), 0, st, X, nj, nc, no, nv, *ga,
                           op_mo, zj, dimr, lr.b[1].off, lr.b[2].off, lr.b[3].off, y, diml, ll.o4);
      HIPCHK(what, hipGetLastError());
      for (long i0 = 0; i0 < nl; i0 += ns) {
        const long ni = nl - i0 < ns ? nl - i0 : ns;
        const double* zi = zj;
        if (gl != gr || i0 != j0) RET(load_chunk(gl, i0, ni, b_zi, &zi));
        GemmDesc g;   // T[x, L, R] = <z_L, Y[x, R]>
        g.M = (int)ni; g.N = (int)nj; g.K = (int)diml; g.nb1 = X;
        g.A = zi; g.sAm = diml; g.sAk = 1;
        g.B = y; g.sBk = 1; g.sBn = diml; g.sBb1 = sy;
        g.C = outd + (first[gl] + i0) * n + (first[gr] + j0); g.ldc = n; g.sCb1 = n * n;
        RET(run(g));
      }
    }
    return 0;
  };

  // ---- the reference state against group grp: as the ket (a column) or the bra (a row) ----
  auto ground = [&](int grp, bool column, const std::vector<Img>& imgs) -> int {
    const long ng = cnt[grp];
    if (!G || ng < 1) return 0;
    const Layout& l = lay[grp];
    RET(b_img.ensure((size_t)X * l.dim, what));
    RET(b_g.ensure((size_t)X * ng, what));
    HIPCHK(what, hipMemsetAsync(b_img.p, 0, (size_t)X * l.dim * 8, st));
    for (const Img& im : imgs) {
      const Blk& b = l.b[im.blk];
      const long rc = (long)kn[b.rk] * kn[b.ck];
      if (rc < 1 || im.f == 0.0) continue;
      const double* m; long sr, sc;
      opblock(b.rk, b.ck, im.tr, &m, &sr, &sc);
      hipLaunchKernelGGL(k_si_image, dim3(nblocks((long)X * rc)), dim3(256), 0, st, X, kn[b.rk], kn[b.ck], sr, sc, nmo2,
                         im.f, m, b_img.p + b.off, l.dim);
    }
    HIPCHK(what, hipGetLastError());
    for (long j0 = 0; j0 < ng; j0 += ns) {
      const long nj = ng - j0 < ns ? ng - j0 : ns;
      const double* zj = nullptr;
      RET(load_chunk(grp, j0, nj, b_zj, &zj));
      GemmDesc g;   // g[x, R] = <image[x], z_R>
      g.M = X; g.N = (int)nj; g.K = (int)l.dim;
      g.A = b_img.p; g.sAm = l.dim; g.sAk = 1;
      g.B = zj; g.sBk = 1; g.sBn = l.dim;
      g.C = b_g.p + j0; g.ldc = ng;
      RET(run(g));
    }
    double* o = column ? outd + first[grp] * n + first[1] : outd + first[1] * n + first[grp];
    hipLaunchKernelGGL(k_si_place, dim3(nblocks((long)X * ng)), dim3(256), 0, st, X, ng, b_g.p, ng, o, n * n,
                       column ? n : 1L);
    HIPCHK(what, hipGetLastError());
    return 0;
  };

  const double r2 = M_SQRT2, h2 = M_SQRT1_2;
  const int L = 0, R = 1, P = 0, T = 1;   // side; plain / transposed block
  if (soc) {
    if (cnt[0] > 0) {   // S >= 1
      const double f1 = (1 - S) / (S * r2), f2 = sqrt((2 * S + 1) / S) * (1 - S) / (2 * S);
      const double f11 = -(S - 1) / (S * r2), w11 = (2 * S + 1) / (2 * S - 1);
      const double f13 = -(S - 1) / sqrt(S * (2 * S - 1)), f14 = -1.0 / (2 * sqrt(S * (2 * S - 1)));
      const double f21 = (1 - S) / sqrt(S * (2 * S - 1)), f28 = -h2;
      const double ga = (1 - S) / S, gb = 2 * (S - 1);   // (1-S)/S + 2(S-1) delta
      const std::vector<Term> mm = {   // interact_S_1S_1, cases 1-35
        {0, 0, R, T, f1}, {0, 0, L, T, f1}, {0, 1, R, T, f2}, {0, 2, L, T, f2},
        {1, 0, R, P, -f2}, {1, 1, L, T, f11}, {1, 1, R, T, f11 * w11}, {1, 3, L, T, f13},
        {2, 0, L, P, -f2}, {2, 2, R, T, f11}, {2, 2, L, T, f11 * w11}, {2, 3, R, T, f21},
        {3, 1, L, P, -f13}, {3, 2, R, P, -f21}, {3, 3, L, T, f28}, {3, 3, R, T, f28}};
      const OSpread sp = {f14 * ga, f14 * gb, f14 * ga, f14 * gb, f28, f28, -f28 / S};
      const OGather og = {-f14 * gb, -f14 * ga, -f14 * gb, -f14 * ga, -f28, -f28, f28 / S,
                          (long)nc * nmo, nmo, 1, ((long)nc + no) * nmo + nc, 1, nmo, 1};
      RET(couple(0, 0, mm, &sp, &og));
      // interact_S_1GS, cases 6, 15, 23, 30
      RET(ground(0, true, {{0, T, sqrt((2 * S - 1) / (2 * S + 1))}, {1, T, sqrt((2 * S - 1) / (2 * S))},
                           {2, T, sqrt((2 * S - 1) / (2 * S))}, {3, T, 1.0}}));
      const double q = sqrt((2 * S - 1) / (2 * S + 1));
      const double f7 = q / r2, f8 = -q / (2 * S), f10 = -sqrt((1 + S) * (2 * S - 1) / (2 * S * (2 * S + 1)));
      const double f16 = sqrt((2 * S - 1) / S) / 2, f17 = -sqrt((2 * S - 1) / (2 * S));
      const double f19 = -sqrt((1 + S) * (2 * S - 1)) / (2 * S);
      const std::vector<Term> mo = {   // interact_S_1S, cases 7-40
        {0, 0, R, T, f7}, {0, 0, L, T, -f7}, {0, 1, R, T, f8}, {0, 2, L, T, -f8}, {0, 3, R, T, f10}, {0, 3, L, T, f10},
        {1, 0, R, T, f16}, {1, 1, L, T, f17}, {1, 1, R, T, f17 / (2 * S - 1)}, {1, 3, R, T, f19},
        {2, 0, L, T, -f16}, {2, 2, R, T, -f17}, {2, 2, L, T, -f17 / (2 * S - 1)}, {2, 3, L, T, f19},
        {3, 1, L, T, -1.0}, {3, 2, R, T, 1.0}};
      const OGather og2 = {-1.0, 1 / (2 * S), 1.0, -1 / (2 * S), 0.0, 0.0, 0.0,
                           (long)nc, 1, nmo, (long)nc * nmo + nc + no, nmo, 1, 0};
      RET(couple(0, 2, mo, nullptr, &og2));
    }
    // interact_GSS, cases 43-45; interact_GSS1, case 46
    RET(ground(2, false, {{1, P, -h2}, {2, P, h2}, {3, P, open ? -sqrt(S / (1 + S)) : 0.0}}));
    RET(ground(3, false, {{0, P, -1.0}}));
    {
      const double f50 = open ? -sqrt(S / (2 * (1 + S))) : 0.0;
      const double f54 = open ? (1 - S) / (2 * sqrt(S * (S + 1))) : 0.0, f59 = open ? 1 / (r2 * (1 + S)) : 0.0;
      const std::vector<Term> ss = {   // interact_SS, cases 47-59 (50, 54, 57, 59 with S != 0 only)
        {0, 1, R, T, -0.5}, {0, 2, L, T, -0.5}, {0, 3, R, T, f50}, {0, 3, L, T, -f50},
        {1, 0, R, P, 0.5}, {1, 1, R, T, -h2}, {1, 1, L, T, h2}, {1, 3, R, T, f54},
        {2, 0, L, P, 0.5}, {2, 2, R, T, h2}, {2, 2, L, T, -h2}, {2, 3, L, T, -f54},
        {3, 0, R, P, -f50}, {3, 0, L, P, f50}, {3, 1, R, P, -f54}, {3, 2, L, P, f54},
        {3, 3, R, T, f59}, {3, 3, L, T, f59}};
      RET(couple(2, 2, ss, nullptr, nullptr));
      const std::vector<Term> sp1 = {   // interact_SS1, cases 51, 55, 58, 60
        {0, 0, L, T, h2}, {0, 0, R, T, -h2}, {1, 0, R, T, -1.0}, {2, 0, L, T, 1.0},
        {3, 0, L, T, f50}, {3, 0, R, T, f50}};
      RET(couple(2, 3, sp1, nullptr, nullptr));
      RET(couple(3, 3, {{0, 0, R, T, h2}, {0, 0, L, T, h2}}, nullptr, nullptr));   // interact_S1S1, case 61
    }
  } else {
    if (cnt[0] > 0) {   // TDM_S_1, tdm.py:156-238
      const double f = sqrt((2 * S + 1) / (2 * S)), f16 = -sqrt(2 * S / (2 * S - 1));
      const double f18 = 1 / sqrt(2 * S * (2 * S - 1));
      const std::vector<Term> mm = {
        {0, 0, R, T, 1.0}, {0, 0, L, T, -1.0}, {1, 1, R, T, 1.0}, {1, 1, L, T, -1.0},
        {2, 2, R, T, 1.0}, {2, 2, L, T, -1.0}, {3, 3, R, T, 1.0}, {3, 3, L, T, -1.0},
        {0, 1, R, T, f}, {1, 0, R, P, f}, {0, 2, L, T, -f}, {2, 0, L, P, -f},
        {1, 3, L, T, f16}, {3, 1, L, P, f16}, {2, 3, R, T, -f16}, {3, 2, R, P, -f16}};
      const OSpread sp = {0.0, -2 * S * f18, 0.0, 2 * S * f18, -1.0, 1.0, 0.0};
      const OGather og = {-2 * S * f18, 0.0, 2 * S * f18, 0.0, -1.0, 1.0, 0.0,
                          (long)nc * nmo, nmo, 1, ((long)nc + no) * nmo + nc, 1, nmo, 1};
      RET(couple(0, 0, mm, &sp, &og));
    }
    RET(ground(2, false, {{0, T, r2}, {1, P, 1.0}, {2, P, 1.0}}));   // TDM_GSS, tdm.py:14-42
    {
      const double g = open ? sqrt((1 + S) / (2 * S)) : 0.0, o = open ? 1.0 : 0.0;
      const std::vector<Term> ss = {   // TDM_S, tdm.py:61-126 (all but case 21 with S != 0 only)
        {0, 0, R, P, 1.0}, {0, 0, L, T, -1.0}, {1, 1, R, P, o}, {1, 1, L, T, -o},
        {2, 2, R, T, o}, {2, 2, L, P, -o}, {3, 3, R, T, o}, {3, 3, L, T, -o},
        {0, 1, R, T, o * h2}, {1, 0, R, P, o * h2}, {0, 2, L, T, -o * h2}, {2, 0, L, P, -o * h2},
        {1, 3, R, T, g}, {3, 1, R, P, g}, {2, 3, L, T, g}, {3, 2, L, P, g}};
      RET(couple(2, 2, ss, nullptr, nullptr));
    }
    RET(couple(3, 3, {{0, 0, R, T, 1.0}, {0, 0, L, T, -1.0}}, nullptr, nullptr));   // TDM_S1, tdm.py:128-154
  }
  if (host) HIPCHK(what, hipMemcpyAsync(out, outd, (size_t)X * n * n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(what, hipStreamSynchronize(st));   // the workspace is released on return
  return 0;
}
