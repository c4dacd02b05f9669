// VV10 non-local correlation: the pair sums of the ground state and of the response
// (xt_vv10_ground, xt_vv10_response; include/xtddft_amd.h), the term the reference adds with
// get_vnlc_resp (xtddft/XTDA.py:515-517).
//
// Energy (a_i = w_i rho_i, points with rho_i > rho_min only):
//   E = sum_i a_i [beta + 1/2 sum_j a_j phi(g_ij, g_ji)],  phi(x, y) = -3/2 / (x y (x + y)),
//   g_ij = omega_i R_ij^2 + kappa_i.
// Per point the energy depends on p_i = (a_i, kappa_i, omega_i); its second derivative splits
// into a pair part, a 3 x 3 block per pair built from phi, phi_x, phi_y, phi_xy, R^2, R^4 acting
// on the sources s1 = da_j, s2 = a_j dkappa_j, s3 = a_j domega_j,
//   out_a_i = sum_j [phi s1 + phi_y (s2 + R^2 s3)]
//   out_k_i = sum_j [phi_x s1 + phi_xy (s2 + R^2 s3)]       (x a_i)
//   out_w_i = sum_j R^2 [phi_x s1 + phi_xy (s2 + R^2 s3)]   (x a_i)
// and a per-point diagonal part from the ground-state sums of xt_vv10_ground
//   F = sum a_j phi,  U = -sum a_j phi_x / 1.5,  W = -sum a_j phi_x R^2 / 1.5,
//   S0, S1, S2 = sum a_j phi_xx {1, R^2, R^4},
// followed by the chain rule to (rho, gamma) in the epilogue.
//
// One kernel shape for both: a block owns 64 target points (one per lane); the sources run in
// tiles of 64 staged in LDS (per-point parameters computed while staging), each of the block's
// four waves taking 16 sources of every tile, so all lanes of a wave read the same source (LDS
// broadcast).  One reciprocal per pair (1 / (x y (x + y))); 1/x, 1/y, 1/(x + y) follow by
// multiplication.  The response keeps 3 accumulators per trial vector in registers for a tile
// of NZB vectors (1, 4, 8, 16 or 24), so a pair's kernel values are generated once per vector
// tile.  The four waves' partial sums are added in fixed order through LDS: same input, same bits.
#include "xt_internal.h"
#include "../../include/xtddft_amd.h"

namespace {

constexpr int TT = 64;    // target points per block (one per lane)
constexpr int TS = 64;    // source points per LDS tile (16 per wave)
constexpr int NW = 4;     // waves per block
constexpr double C43 = 4.18879020478639098461685784437;   // 4 pi / 3
constexpr double KPREF = 2.6998671913905572;              // (3/2) pi (9 pi)^(-1/6)

struct Point {
  double a, ka, om, w, kr, omr, omg;
};

// per-point parameters and first derivatives; a masked point is a source of weight zero with
// finite (kappa, omega) = (1, 1), so every pair value stays finite
__device__ __forceinline__ Point point_of(bool act, double rho, double gam, double w, double b, double C) {
  Point p = {0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0};
  if (!act) return p;
  const double r2 = rho * rho, r4 = r2 * r2, cg = C * gam;
  const double om = sqrt(cg * gam / r4 + C43 * rho);
  p.a = w * rho;
  p.ka = b * KPREF * cbrt(sqrt(rho));
  p.om = om;
  p.w = w;
  p.kr = p.ka / (6.0 * rho);
  p.omr = (-4.0 * cg * gam / (r4 * rho) + C43) / (2.0 * om);
  p.omg = (2.0 * cg / r4) / (2.0 * om);
  return p;
}

struct Args {
  int G, i0, i1, nz;
  const double* xyz; const double* w; const double* rho; const double* gam;
  double b, C, rho_min;
  const double* sums;       // response: (6, G) from the ground kernel
  const double* rho1; const double* gam1;
  double* o0; double* o1;   // ground: o0 = sums (6, G); response: vrho1, vgamma1 (nz, G)
};

// NZB = 0: the ground-state sums
template <int NZB>
__global__ __launch_bounds__(TT * NW) void k_vv10(const Args q) {
  constexpr int NACC = NZB == 0 ? 6 : 3 * NZB;
  constexpr int NSRC = NZB == 0 ? 6 : 10 + 3 * NZB;   // doubles per source in the tile
  constexpr int NSM = (NSRC > NACC ? NSRC : NACC) * TS;
  __shared__ double sm[NSM];
  const int tid = threadIdx.x, t = tid & 63, sl = tid >> 6;
  const int G = q.G;
  const int i = q.i0 + blockIdx.x * TT + t;
  const int v0 = blockIdx.y * NZB;
  const bool in_win = i < q.i1;
  double xi = 0.0, yi = 0.0, zi = 0.0;
  bool act_i = false;
  double rho_i = 1.0, gam_i = 0.0, w_i = 0.0;
  if (in_win) {
    xi = q.xyz[3 * (size_t)i]; yi = q.xyz[3 * (size_t)i + 1]; zi = q.xyz[3 * (size_t)i + 2];
    rho_i = q.rho[i]; gam_i = q.gam[i]; w_i = q.w[i];
    act_i = rho_i > q.rho_min;
  }
  const Point pi = point_of(act_i, rho_i, gam_i, w_i, q.b, q.C);
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;

  double* sx = sm; double* sy = sm + TS; double* sz = sm + 2 * TS;
  double* sa = sm + 3 * TS; double* sk = sm + 4 * TS; double* so = sm + 5 * TS;
  for (int j0 = 0; j0 < G; j0 += TS) {
    __syncthreads();   // the previous tile is consumed
    if (tid < TS) {
      const int j = j0 + tid;
      double x = 0.0, y = 0.0, z = 0.0, rho = 1.0, gam = 0.0, w = 0.0;
      bool act = false;
      if (j < G) {
        x = q.xyz[3 * (size_t)j]; y = q.xyz[3 * (size_t)j + 1]; z = q.xyz[3 * (size_t)j + 2];
        rho = q.rho[j]; gam = q.gam[j]; w = q.w[j];
        act = rho > q.rho_min;
      }
      const Point p = point_of(act, rho, gam, w, q.b, q.C);
      sx[tid] = x; sy[tid] = y; sz[tid] = z; sa[tid] = p.a; sk[tid] = p.ka; so[tid] = p.om;
      if constexpr (NZB > 0) {
        sm[6 * TS + tid] = p.w; sm[7 * TS + tid] = p.kr; sm[8 * TS + tid] = p.omr; sm[9 * TS + tid] = p.omg;
      }
    }
    if constexpr (NZB > 0) {
      __syncthreads();
      for (int e = tid; e < NZB * TS; e += TT * NW) {
        const int jj = e & (TS - 1), v = e / TS;
        const int j = j0 + jj, vv = v0 + v;
        double d1 = 0.0, g1 = 0.0;
        if (j < G && vv < q.nz) { d1 = q.rho1[(size_t)vv * G + j]; g1 = q.gam1[(size_t)vv * G + j]; }
        const double a = sa[jj];
        double* s = sm + (10 + 3 * v) * TS + jj;
        s[0] = sm[6 * TS + jj] * d1;
        s[TS] = a * sm[7 * TS + jj] * d1;
        s[2 * TS] = a * (sm[8 * TS + jj] * d1 + sm[9 * TS + jj] * g1);
      }
    }
    __syncthreads();
    const int jb = sl * (TS / NW);
    for (int jj = jb; jj < jb + TS / NW; ++jj) {
      const double dx = xi - sx[jj], dy = yi - sy[jj], dz = zi - sz[jj];
      const double R2 = dx * dx + dy * dy + dz * dz;
      const double x = pi.om * R2 + pi.ka, y = so[jj] * R2 + sk[jj];
      const double s = x + y, xy = x * y;
      const double r = 1.0 / (xy * s);
      const double is = xy * r, ix = y * s * r;
      const double ux = ix + is;
      if constexpr (NZB == 0) {
        const double T = sa[jj] * r, tu = T * ux;
        const double pxx = -1.5 * T * (ux * ux + ix * ix + is * is);
        acc[0] += T; acc[1] += tu; acc[2] += R2 * tu;
        acc[3] += pxx; acc[4] += R2 * pxx; acc[5] += R2 * R2 * pxx;
      } else {
        const double uy = x * s * r + is;
        const double phi = -1.5 * r, phx = -phi * ux, phy = -phi * uy, phxy = phi * (ux * uy + is * is);
#pragma unroll
        for (int v = 0; v < NZB; ++v) {
          const double* sv = sm + (10 + 3 * v) * TS + jj;
          const double s1 = sv[0], tt = sv[TS] + R2 * sv[2 * TS];
          const double bv = phx * s1 + phxy * tt;
          acc[3 * v] += phi * s1 + phy * tt;
          acc[3 * v + 1] += bv;
          acc[3 * v + 2] += R2 * bv;
        }
      }
    }
  }
  // the four waves' partial sums, added in wave order
  for (int s = 1; s < NW; ++s) {
    __syncthreads();
    if (sl == s) {
#pragma unroll
      for (int k = 0; k < NACC; ++k) sm[k * TS + t] = acc[k];
    }
    __syncthreads();
    if (sl == 0) {
#pragma unroll
      for (int k = 0; k < NACC; ++k) acc[k] += sm[k * TS + t];
    }
  }
  if (sl != 0 || !in_win) return;
  if constexpr (NZB == 0) {
    const double f[6] = {-1.5 * acc[0], acc[1], acc[2], acc[3], acc[4], acc[5]};
#pragma unroll
    for (int k = 0; k < 6; ++k) q.o0[(size_t)k * G + i] = act_i ? f[k] : 0.0;
  } else {
  // chain rule to (rho, gamma): second derivatives of kappa and omega at the target
  const double P = 1.5 * q.sums[(size_t)G + i], Q = 1.5 * q.sums[2 * (size_t)G + i];
  const double S0 = q.sums[3 * (size_t)G + i], S1 = q.sums[4 * (size_t)G + i], S2 = q.sums[5 * (size_t)G + i];
  const double r2 = rho_i * rho_i, r4 = r2 * r2, cg = q.C * gam_i;
  const double q_r = -4.0 * cg * gam_i / (r4 * rho_i) + C43, q_g = 2.0 * cg / r4;
  const double h = 1.0 / (2.0 * pi.om), h3 = h / (2.0 * pi.om * pi.om);   // 1/(2 om), 1/(4 om^3)
  const double krr = -5.0 * pi.ka / (36.0 * r2);
  const double omrr = 20.0 * cg * gam_i / (r4 * r2) * h - q_r * q_r * h3;
  const double omrg = -8.0 * cg / (r4 * rho_i) * h - q_r * q_g * h3;
  const double omgg = 2.0 * q.C / r4 * h - q_g * q_g * h3;
  const double a = pi.a;
#pragma unroll
  for (int v = 0; v < NZB; ++v) {
    const int vv = v0 + v;
    if (vv >= q.nz) break;
    double vr = 0.0, vg = 0.0;
    if (act_i) {
      const double d1 = q.rho1[(size_t)vv * G + i], g1 = q.gam1[(size_t)vv * G + i];
      const double da = pi.w * d1, dk = pi.kr * d1, dom = pi.omr * d1 + pi.omg * g1;
      const double dEa = acc[3 * v] + P * dk + Q * dom;
      const double dEk = P * da + a * (acc[3 * v + 1] + S0 * dk + S1 * dom);
      const double dEw = Q * da + a * (acc[3 * v + 2] + S1 * dk + S2 * dom);
      vr = pi.w * dEa + pi.kr * dEk + pi.omr * dEw + a * P * krr * d1 + a * Q * (omrr * d1 + omrg * g1);
      vg = pi.omg * dEw + a * Q * (omrg * d1 + omgg * g1);
    }
    q.o0[(size_t)vv * G + i] = vr;
    q.o1[(size_t)vv * G + i] = vg;
  }
  }
}

int check_common(int G, const double* xyz, const double* w, const double* rho, const double* gam, double b, double C,
                 double rho_min, int i0, int i1) {
  if (G < 0 || i0 < 0 || i0 > i1 || i1 > G) return xt::set_error(XT_ERR_ARG, "vv10: need 0 <= i0 <= i1 <= ngrid");
  if (!(b > 0.0) || !(C >= 0.0) || !(rho_min >= 0.0))
    return xt::set_error(XT_ERR_ARG, "vv10: need b > 0, C >= 0, rho_min >= 0");
  if (i1 > i0 && (!xyz || !w || !rho || !gam)) return xt::set_error(XT_ERR_ARG, "vv10: null grid array");
  return 0;
}

template <int NZB>
int launch(const Args& q, hipStream_t st) {
  const dim3 grid((q.i1 - q.i0 + TT - 1) / TT, NZB == 0 ? 1 : (q.nz + NZB - 1) / NZB);
  hipLaunchKernelGGL(k_vv10<NZB>, grid, dim3(TT * NW), 0, st, q);
  return hipGetLastError() == hipSuccess ? 0 : xt::set_error(XT_ERR_HIP, "vv10 kernel launch failed");
}

}  // namespace

extern "C" int xt_vv10_ground(int ngrid, const double* coords, const double* weights, const double* rho,
                              const double* gamma, double b, double C, double rho_min, int i0, int i1,
                              double* sums, void* hip_stream) {
  const int r = check_common(ngrid, coords, weights, rho, gamma, b, C, rho_min, i0, i1);
  if (r) return r;
  if (i1 == i0) return 0;
  if (!sums) return xt::set_error(XT_ERR_ARG, "vv10: null output");
  Args q = {ngrid, i0, i1, 0, coords, weights, rho, gamma, b, C, rho_min, nullptr, nullptr, nullptr, sums, nullptr};
  return launch<0>(q, (hipStream_t)hip_stream);
}

extern "C" int xt_vv10_response(int ngrid, const double* coords, const double* weights, const double* rho,
                                const double* gamma, double b, double C, double rho_min, const double* sums,
                                int nz, const double* rho1, const double* gamma1, int i0, int i1,
                                double* vrho1, double* vgamma1, void* hip_stream) {
  const int r = check_common(ngrid, coords, weights, rho, gamma, b, C, rho_min, i0, i1);
  if (r) return r;
  if (nz < 0) return xt::set_error(XT_ERR_ARG, "vv10: negative vector count");
  if (i1 == i0 || nz == 0) return 0;
  if (!sums || !rho1 || !gamma1 || !vrho1 || !vgamma1) return xt::set_error(XT_ERR_ARG, "vv10: null argument");
  Args q = {ngrid, i0, i1, nz, coords, weights, rho, gamma, b, C, rho_min, sums, rho1, gamma1, vrho1, vgamma1};
  hipStream_t st = (hipStream_t)hip_stream;
  if (nz <= 1) return launch<1>(q, st);
  if (nz <= 4) return launch<4>(q, st);
  if (nz <= 8) return launch<8>(q, st);
  if (nz <= 16) return launch<16>(q, st);
  return launch<24>(q, st);
}

// ---------------------------------------------------------------------------
// Point kernels of the context's NLC path (xt_set_nlc / xt_apply in xt_ctx.hip).
// MO values on the NLC grid: plane c (value, d/dx, d/dy, d/dz) of point g, orbital p at
// P[c compP + g nmo + p].
// ---------------------------------------------------------------------------
namespace {

// rho0 = sum_occ phi^2 over both spins, grad rho0 = 2 sum_occ phi grad phi, gamma0 = |grad rho0|^2
__global__ void k_vv10_rho0(int n, int nmo, long compP, const double* __restrict__ PA, int nocc_a,
                            const double* __restrict__ PB, int nocc_b, double* __restrict__ rho,
                            double* __restrict__ grad, double* __restrict__ gam) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  double r = 0.0, d[3] = {0.0, 0.0, 0.0};
  for (int s = 0; s < 2; ++s) {
    const double* P = (s == 0 ? PA : PB) + (long)g * nmo;
    const int no = s == 0 ? nocc_a : nocc_b;
    for (int i = 0; i < no; ++i) {
      const double p = P[i];
      r += p * p;
      for (int c = 0; c < 3; ++c) d[c] += 2.0 * p * P[(c + 1) * compP + i];
    }
  }
  rho[g] = r;
  for (int c = 0; c < 3; ++c) grad[(long)c * n + g] = d[c];
  gam[g] = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
}

// dE/dgamma_i = a_i 3/2 W_i domega0/dgamma
__global__ void k_vv10_vgamma0(int n, const double* __restrict__ w, const double* __restrict__ rho,
                               const double* __restrict__ gam, const double* __restrict__ sums, double b, double C,
                               double rho_min, double* __restrict__ vg) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const Point p = point_of(rho[g] > rho_min, rho[g], gam[g], w[g], b, C);
  vg[g] = p.a * 1.5 * sums[2 * (long)n + g] * p.omg;
}

struct Spin2 { const double* P[2]; double* U[2]; long ld[2]; };

// rho1[x, g] = sum_s sum_i phi_i U0[g, (x, i)], grad rho1_c = sum_s sum_i (d_c phi_i U0 + phi_i Uc),
// gamma1 = 2 grad rho0 . grad rho1; U planes tcs apart
__global__ void k_vv10_forward(int n, int g0, int Gn, int nz, int O, int nmo, long compP, Spin2 q, long tcs,
                               const double* __restrict__ grad0, double* __restrict__ rho1,
                               double* __restrict__ gam1, double* __restrict__ grad1) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)n * nz) return;
  const int x = (int)(t % nz), g = (int)(t / nz);
  double r = 0.0, d[3] = {0.0, 0.0, 0.0};
  for (int s = 0; s < 2; ++s) {
    const double* P = q.P[s] + (long)g * nmo;
    const double* U = q.U[s] + (long)g * q.ld[s] + (long)x * O;
    for (int i = 0; i < O; ++i) {
      const double p = P[i], u = U[i];
      r += p * u;
      for (int c = 0; c < 3; ++c) d[c] += P[(c + 1) * compP + i] * u + p * U[(c + 1) * tcs + i];
    }
  }
  const long o = (long)x * Gn + g0 + g;
  rho1[o] = r;
  double gm = 0.0;
  for (int c = 0; c < 3; ++c) {
    grad1[((long)c * nz) * Gn + o] = d[c];
    gm += grad0[(long)c * Gn + g0 + g] * d[c];
  }
  gam1[o] = 2.0 * gm;
}

// L0[g, (x, i)] = wv0 phi_i + sum_c wv_c d_c phi_i,  Lc[g, (x, i)] = wv_c phi_i, with wv0 = vrho1,
// wv_c = 2 vgamma1 grad rho0_c + 2 dE/dgamma grad rho1_c (the same for both spins)
__global__ void k_vv10_back_l(int n, int g0, int Gn, int nz, int O, int nmo, long compP, Spin2 q, long tcs,
                              const double* __restrict__ grad0, const double* __restrict__ vg0,
                              const double* __restrict__ vr1, const double* __restrict__ vg1,
                              const double* __restrict__ grad1) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2L * n * nz * O) return;
  const int i = (int)(t % O);
  long r = t / O;
  const int x = (int)(r % nz); r /= nz;
  const int g = (int)(r % n), s = (int)(r / n);
  const long o = (long)x * Gn + g0 + g;
  const double* P = q.P[s] + (long)g * nmo + i;
  double* L = q.U[s] + (long)g * q.ld[s] + (long)x * O + i;
  const double p = P[0];
  double l0 = vr1[o] * p;
  for (int c = 0; c < 3; ++c) {
    const double wv = 2.0 * vg1[o] * grad0[(long)c * Gn + g0 + g] + 2.0 * vg0[g0 + g] * grad1[((long)c * nz) * Gn + o];
    l0 += wv * P[(c + 1) * compP];
    L[(c + 1) * tcs] = wv * p;
  }
  L[0] = l0;
}

inline unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

namespace xt {

void vv10_rho0(hipStream_t st, int n, int nmo, long compP, const double* PA, int nocc_a, const double* PB,
               int nocc_b, double* rho, double* grad, double* gam) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_vv10_rho0, dim3(blocks_of(n)), dim3(256), 0, st, n, nmo, compP, PA, nocc_a, PB, nocc_b, rho,
                     grad, gam);
}

void vv10_vgamma0(hipStream_t st, int n, const double* w, const double* rho, const double* gam, const double* sums,
                  double b, double C, double rho_min, double* vg) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_vv10_vgamma0, dim3(blocks_of(n)), dim3(256), 0, st, n, w, rho, gam, sums, b, C, rho_min, vg);
}

void vv10_forward(hipStream_t st, int n, int g0, int Gn, int nz, int O, int nmo, long compP, const double* P0,
                  const double* P1, double* U0, long ld0, double* U1, long ld1, long tcs, const double* grad0,
                  double* rho1, double* gam1, double* grad1) {
  if (n <= 0 || nz <= 0) return;
  const Spin2 q = {{P0, P1}, {U0, U1}, {ld0, ld1}};
  hipLaunchKernelGGL(k_vv10_forward, dim3(blocks_of((long)n * nz)), dim3(256), 0, st, n, g0, Gn, nz, O, nmo, compP,
                     q, tcs, grad0, rho1, gam1, grad1);
}

void vv10_back_l(hipStream_t st, int n, int g0, int Gn, int nz, int O, int nmo, long compP, const double* P0,
                 const double* P1, double* L0, long ld0, double* L1, long ld1, long tcs, const double* grad0,
                 const double* vg0, const double* vr1, const double* vg1, const double* grad1) {
  if (n <= 0 || nz <= 0) return;
  const Spin2 q = {{P0, P1}, {L0, L1}, {ld0, ld1}};
  hipLaunchKernelGGL(k_vv10_back_l, dim3(blocks_of(2L * n * nz * O)), dim3(256), 0, st, n, g0, Gn, nz, O, nmo,
                     compP, q, tcs, grad0, vg0, vr1, vg1, grad1);
}

}  // namespace xt
