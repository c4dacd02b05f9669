// xt_tdm: state-to-state transition moments of spin-flip amplitudes
// (include/xtddft_amd.h; XSF_TDA.calculate_TDM_R / calculate_TDM_U, XSF_TDA.py:435-592).
//
// The reference evaluates 16 trace terms per ordered pair of states and component.  They
// are bilinear in the two states, T_x[i,j] = <c_i, D_x c_j>, so here D_x is applied once to
// every state and one Gram product gives all pairs:
//
//   D_occ[x] = Cocc^T op_x Cocc, D_vir[x] = Cvir^T op_x Cvir        engine GEMMs
//   images D^(f1), D^(f2) (off-diagonal blocks scaled)               k_tdm_images
//   c[s] (O x V) from the vector rows, OO expanded by vects          k_tdm_pack
//   Y[x,s] = c[s] D_vir^(f) - D_occ^(f) c[s]                         engine GEMMs (row / column blocks)
//   the f3 terms: tr(oo), sum D[c,o] o co, sum D[o,v] o ov           k_tdm_f3 (fixed-order tree)
//   T[x] = C Y[x]^T                                                  engine GEMM over dim
//
// States are processed in chunks so that the buffers growing with nstates (c of two
// chunks, Y, the upload stage) stay within a fixed budget; every product has a shape that
// depends only on the descriptor, so the split-K plans and with them the bits repeat.
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

// d1 = d with the off-diagonal blocks (row < split) != (col < split) times f1, d2 with f2;
// nmat matrices of n x n
__global__ void k_tdm_images(long nmat, int n, int split, double f1, double f2, const double* __restrict__ d,
                             double* __restrict__ d1, double* __restrict__ d2) {
  GRID_STRIDE(t, nmat * n * n) {
    const int c = (int)(t % n), r = (int)((t / n) % n);
    const bool off = (r < split) != (c < split);
    const double v = d[t];
    d1[t] = off ? f1 * v : v;
    d2[t] = off ? f2 * v : v;
  }
}

// cv|co|ov|oo rows (dim doubles each) -> c (O x V): rows [c|o], columns [o|v]; a compressed
// OO block (no^2 - 1 coefficients) is expanded by vects (no^2 x (no^2 - 1)), oo = vects w
// (XSF_TDA.py:509-515).  blockIdx.y = state.
__global__ void k_tdm_pack(int nc, int no, int nv, int compressed, long dim, const double* __restrict__ vects,
                           const double* __restrict__ vecs, double* __restrict__ c) {
  const int O = nc + no, V = no + nv;
  const long d1 = (long)nc * nv, d2 = d1 + (long)nc * no, d3 = d2 + (long)no * nv;
  const double* z = vecs + blockIdx.y * dim;
  double* cs = c + (long)blockIdx.y * O * V;
  GRID_STRIDE(t, (long)O * V) {
    const int a = (int)(t % V), i = (int)(t / V);
    double v;
    if (i < nc) {
      v = a >= no ? z[(long)i * nv + (a - no)] : z[d1 + (long)i * no + a];
    } else {
      const int u = i - nc;
      if (a >= no) {
        v = z[d2 + (long)u * nv + (a - no)];
      } else if (compressed) {
        const int m = no * no - 1;
        const double* row = vects + (long)(u * no + a) * m;
        v = 0.0;
        for (int y = 0; y < m; ++y) v += row[y] * z[d3 + y];
      } else {
        v = z[d3 + u * no + a];
      }
    }
    cs[t] = v;
  }
}

// The f3 terms of one (state, component) per block (XSF_TDA.py:557, 563, 576, 582):
//   Y_co += f3 tr(oo) D_occ[c,o],  Y_ov -= f3 tr(oo) D_vir[o,v],
//   Y_oo += f3 I (sum D_occ[c,o] o co - sum D_vir[o,v] o ov)
// with the un-scaled D.  Each thread sums a fixed stride of the terms, then a fixed tree
// over the block: no atomics, the same bits every call.  grid (ns, ncomp), 256 threads.
__global__ void __launch_bounds__(256) k_tdm_f3(int nc, int no, int nv, double f3, const double* __restrict__ docc,
                                                const double* __restrict__ dvir, const double* __restrict__ c,
                                                double* __restrict__ y) {
  __shared__ double red[2][256];
  const int O = nc + no, V = no + nv, tid = threadIdx.x;
  const long ov = (long)O * V;
  const double* cs = c + blockIdx.x * ov;
  double* ys = y + ((long)blockIdx.y * gridDim.x + blockIdx.x) * ov;
  const double* dO = docc + (long)blockIdx.y * O * O;
  const double* dV = dvir + (long)blockIdx.y * V * V;
  const int nco = nc * no, nov = no * nv;
  double s = 0.0, tr = 0.0;
  for (int k = tid; k < nco; k += 256) {
    const int i = k / no, u = k % no;
    s += dO[(long)i * O + nc + u] * cs[(long)i * V + u];
  }
  for (int k = tid; k < nov; k += 256) {
    const int u = k / nv, a = k % nv;
    s -= dV[(long)u * V + no + a] * cs[(long)(nc + u) * V + no + a];
  }
  for (int u = tid; u < no; u += 256) tr += cs[(long)(nc + u) * V + u];
  red[0][tid] = s;
  red[1][tid] = tr;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) { red[0][tid] += red[0][tid + w]; red[1][tid] += red[1][tid + w]; }
    __syncthreads();
  }
  s = f3 * red[0][0];
  tr = f3 * red[1][0];
  for (int k = tid; k < nco; k += 256) {
    const int i = k / no, u = k % no;
    ys[(long)i * V + u] += tr * dO[(long)i * O + nc + u];
  }
  for (int k = tid; k < nov; k += 256) {
    const int u = k / nv, a = k % nv;
    ys[(long)(nc + u) * V + no + a] -= tr * dV[(long)u * V + no + a];
  }
  for (int u = tid; u < no; u += 256) ys[(long)(nc + u) * V + u] += s;
}

const char* const what = "xt_tdm";   // message prefix

}  // namespace

extern "C" int xt_tdm(const xt_tdm_desc* desc, const double* op_ao, const double* c_occ, const double* c_vir,
                      const double* vecs, const double* vects, double* out, int ptr_kind, void* stream) {
  // ---- validation: before any HIP call ----
  if (!desc) return set_error(XT_ERR_ARG, "xt_tdm: null descriptor");
  const xt_tdm_desc d = *desc;
  if (d.ncomp < 1) return set_error(XT_ERR_ARG, "xt_tdm: ncomp < 1");
  if (d.nstates < 1) return set_error(XT_ERR_ARG, "xt_tdm: nstates < 1");
  if (d.layout != XT_TDM_LAYOUT_OV && d.layout != XT_TDM_LAYOUT_BLOCKS)
    return set_error(XT_ERR_ARG, "xt_tdm: unknown layout");
  if (d.nao < 1 || d.nc < 0 || d.no < 0 || d.nv < 0 || d.nc + d.no < 1 || d.no + d.nv < 1)
    return set_error(XT_ERR_ARG, "xt_tdm: bad orbital counts (need nao >= 1, nc + no >= 1, no + nv >= 1)");
  if (d.oo_compressed && d.layout != XT_TDM_LAYOUT_BLOCKS)
    return set_error(XT_ERR_ARG, "xt_tdm: OO compression belongs to the block layout");
  if (d.oo_compressed && (d.no < 1 || (!vects && d.no > 1)))
    return set_error(XT_ERR_ARG, "xt_tdm: OO compression needs an open shell and the basis vects");
  if (d.sa != 0 && 2.0 * d.si - 1.0 <= 0.0)
    return set_error(XT_ERR_ARG, "xt_tdm: spin adaptation needs 2S-1 > 0");
  if (!op_ao || !c_occ || !c_vir || !vecs || !out) return set_error(XT_ERR_ARG, "xt_tdm: null argument");
  if (ptr_kind != XT_PTR_HOST && ptr_kind != XT_PTR_DEVICE) return set_error(XT_ERR_ARG, "xt_tdm: bad ptr_kind");

  hipStream_t st = (hipStream_t)stream;
  const bool host = ptr_kind == XT_PTR_HOST;
  const bool blocks = d.layout == XT_TDM_LAYOUT_BLOCKS;
  const int nc = d.nc, no = d.no, nv = d.nv, X = d.ncomp, N = d.nstates, nao = d.nao;
  const int O = nc + no, V = no + nv;
  const long ov = (long)O * V;
  const long dim = blocks ? (long)nc * nv + (long)nc * no + (long)no * nv + (long)no * no - (d.oo_compressed ? 1 : 0) : ov;
  double f1 = 1.0, f2 = 1.0, f3 = 0.0;
  if (d.sa != 0) {
    const double s2 = 2.0 * d.si;
    f1 = sqrt((s2 + 1.0) / s2); f2 = sqrt(s2 / (s2 - 1.0)); f3 = 1.0 / sqrt(s2 * (s2 - 1.0));
  }
  const bool scaled = d.sa != 0 && no > 0;   // without an open shell no block is scaled

  // states per chunk: c of the column chunk and of the row chunk, Y for every component and
  // the upload stage within the budget (tdm_budget_mib)
  const double per_state = 8.0 * ((double)(X + 2) * ov + (double)dim);
  long ns = (long)(tdm_budget_mib() * 1048576.0 / per_state);
  if (ns > 32768 / X) ns = 32768 / X;   // (state, component) batches of one launch: grid z
  ns = ns < 1 ? 1 : (ns > N ? N : ns);

  // ---- inputs on the device ----
  TmpBuf b_op, b_co, b_cv, b_vt, b_out;
  RET(upload(b_op, op_ao, (size_t)X * nao * nao, ptr_kind, st, what));
  RET(upload(b_co, c_occ, (size_t)nao * O, ptr_kind, st, what));
  RET(upload(b_cv, c_vir, (size_t)nao * V, ptr_kind, st, what));
  if (d.oo_compressed && no > 1) RET(upload(b_vt, vects, (size_t)no * no * (no * no - 1), ptr_kind, st, what));
  double* outd = out;
  if (host) { RET(b_out.ensure((size_t)X * N * N, what)); outd = b_out.p; }

  // ---- engine launches (split-K workspace grown on demand, 256 MiB cap) ----
  TmpBuf ws;
  auto run = [&](const GemmDesc& g) -> int {
    if (g.M <= 0 || g.N <= 0 || g.nb1 <= 0 || g.nb2 <= 0) return 0;   // empty block: nothing is launched
    return run_gemm(g, st, ws, (size_t)256 << 20, 0, what, "GEMM launch failed");
  };

  // ---- D_occ, D_vir for every component ----
  TmpBuf b_half, b_docc, b_dvir, b_img;
  RET(b_half.ensure((size_t)X * nao * (O > V ? O : V), what));
  RET(b_docc.ensure((size_t)X * O * O, what));
  RET(b_dvir.ensure((size_t)X * V * V, what));
  auto to_mo = [&](const double* cm, int n, double* dmo) -> int {
    GemmDesc g;   // half[x] = op[x] C
    g.M = nao; g.N = n; g.K = nao; g.nb1 = X;
    g.A = op_ao; g.sAm = nao; g.sAk = 1; g.sAb1 = (long)nao * nao;
    g.B = cm; g.sBk = n; g.sBn = 1;
    g.C = b_half.p; g.ldc = n; g.sCb1 = (long)nao * n;
    RET(run(g));
    GemmDesc h;   // D[x] = C^T half[x]
    h.M = n; h.N = n; h.K = nao; h.nb1 = X;
    h.A = cm; h.sAm = 1; h.sAk = n;
    h.B = b_half.p; h.sBk = n; h.sBn = 1; h.sBb1 = (long)nao * n;
    h.C = dmo; h.ldc = n; h.sCb1 = (long)n * n;
    return run(h);
  };
  RET(to_mo(c_occ, O, b_docc.p));
  RET(to_mo(c_vir, V, b_dvir.p));
  // factor-scaled images: [D_occ^(f1), D_occ^(f2), D_vir^(f1), D_vir^(f2)]
  const double *do1 = b_docc.p, *do2 = b_docc.p, *dv1 = b_dvir.p, *dv2 = b_dvir.p;
  if (scaled) {
    const size_t so = (size_t)X * O * O, sv = (size_t)X * V * V;
    RET(b_img.ensure(2 * so + 2 * sv, what));
    double* p = b_img.p;
    hipLaunchKernelGGL(k_tdm_images, dim3(nblocks((long)so)), dim3(256), 0, st, (long)X, O, nc, f1, f2, b_docc.p, p, p + so);
    hipLaunchKernelGGL(k_tdm_images, dim3(nblocks((long)sv)), dim3(256), 0, st, (long)X, V, no, f1, f2, b_dvir.p,
                       p + 2 * so, p + 2 * so + sv);
    do1 = p; do2 = p + so; dv1 = p + 2 * so; dv2 = p + 2 * so + sv;
  }

  // ---- state chunks ----
  const bool own_c = host || blocks;          // otherwise a chunk's c is the caller's rows
  TmpBuf b_cj, b_ci, b_stage, b_y;
  if (own_c) RET(b_cj.ensure((size_t)ns * ov, what));
  if (own_c && ns < N) RET(b_ci.ensure((size_t)ns * ov, what));
  if (host && blocks) RET(b_stage.ensure((size_t)ns * dim, what));
  RET(b_y.ensure((size_t)X * ns * ov, what));
  auto load_chunk = [&](long s0, long n, double* buf, const double** c) -> int {
    const double* src = vecs + s0 * dim;
    if (host) {
      double* dst = blocks ? b_stage.p : buf;
      HIPCHK(what, hipMemcpyAsync(dst, src, (size_t)n * dim * 8, hipMemcpyHostToDevice, st));
      src = dst;
    }
    if (blocks) {
      hipLaunchKernelGGL(k_tdm_pack, dim3(nblocks(ov, 256), (unsigned)n), dim3(256), 0, st, nc, no, nv,
                         d.oo_compressed, dim, vects, src, buf);
      src = buf;
    }
    *c = src;
    return 0;
  };

  for (long j0 = 0; j0 < N; j0 += ns) {
    const long nj = N - j0 < ns ? N - j0 : ns;
    const double* cj = nullptr;
    RET(load_chunk(j0, nj, b_cj.p, &cj));
    double* y = b_y.p;
    const long sy = nj * ov;   // component stride of Y
    if (!scaled) {
      GemmDesc g;   // Y[x] = c D_vir[x], the chunk's rows as one matrix
      g.M = (int)(nj * O); g.N = V; g.K = V; g.nb1 = X;
      g.A = cj; g.sAm = V; g.sAk = 1;
      g.B = dv1; g.sBk = V; g.sBn = 1; g.sBb1 = (long)V * V;
      g.C = y; g.ldc = V; g.sCb1 = sy;
      RET(run(g));
      GemmDesc h;   // Y[x,s] -= D_occ[x] c[s]
      h.M = O; h.N = V; h.K = O; h.nb1 = (int)nj; h.nb2 = X;
      h.A = do1; h.sAm = O; h.sAk = 1; h.sAb2 = (long)O * O;
      h.B = cj; h.sBk = V; h.sBn = 1; h.sBb1 = ov;
      h.C = y; h.ldc = V; h.sCb1 = ov; h.sCb2 = sy;
      h.alpha = -1.0; h.beta = 1.0;
      RET(run(h));
    } else {
      for (int part = 0; part < 2; ++part) {   // row blocks c | o: D_vir^(f1) | D_vir^(f2)
        const int r0 = part ? nc : 0, nr = part ? no : nc;
        GemmDesc g;
        g.M = nr; g.N = V; g.K = V; g.nb1 = (int)nj; g.nb2 = X;
        g.A = cj + (long)r0 * V; g.sAm = V; g.sAk = 1; g.sAb1 = ov;
        g.B = part ? dv2 : dv1; g.sBk = V; g.sBn = 1; g.sBb2 = (long)V * V;
        g.C = y + (long)r0 * V; g.ldc = V; g.sCb1 = ov; g.sCb2 = sy;
        RET(run(g));
      }
      for (int part = 0; part < 2; ++part) {   // column blocks o | v: D_occ^(f2) | D_occ^(f1)
        const int c0 = part ? no : 0, ncol = part ? nv : no;
        GemmDesc h;
        h.M = O; h.N = ncol; h.K = O; h.nb1 = (int)nj; h.nb2 = X;
        h.A = part ? do1 : do2; h.sAm = O; h.sAk = 1; h.sAb2 = (long)O * O;
        h.B = cj + c0; h.sBk = V; h.sBn = 1; h.sBb1 = ov;
        h.C = y + c0; h.ldc = V; h.sCb1 = ov; h.sCb2 = sy;
        h.alpha = -1.0; h.beta = 1.0;
        RET(run(h));
      }
      if (f3 != 0.0)
        hipLaunchKernelGGL(k_tdm_f3, dim3((unsigned)nj, (unsigned)X), dim3(256), 0, st, nc, no, nv, f3, b_docc.p,
                           b_dvir.p, cj, y);
    }
    for (long i0 = 0; i0 < N; i0 += ns) {
      const long ni = N - i0 < ns ? N - i0 : ns;
      const double* ci = cj;
      if (i0 != j0) RET(load_chunk(i0, ni, b_ci.p, &ci));
      GemmDesc g;   // T[x, i, j] = sum c[i] o Y[x, j]
      g.M = (int)ni; g.N = (int)nj; g.K = (int)ov; g.nb1 = X;
      g.A = ci; g.sAm = ov; g.sAk = 1;
      g.B = y; g.sBk = 1; g.sBn = ov; g.sBb1 = sy;
      g.C = outd + i0 * N + j0; g.ldc = N; g.sCb1 = (long)N * N;
      RET(run(g));
    }
  }
  HIPCHK(what, hipGetLastError());
  if (host) HIPCHK(what, hipMemcpyAsync(out, outd, (size_t)X * N * N * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(what, hipStreamSynchronize(st));   // the workspace is released on return
  return 0;
}
