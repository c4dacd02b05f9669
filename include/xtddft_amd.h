/* xtddft_amd -- MI355X-native TDA response hot path (C ABI).
 *
 * Drop-in boundary for the Davidson/TDA operator of
 * Quantum-Chemistry-Group-BNU/XTDDFT.  Each entry point names the reference
 * interface it replaces (file:line relative to the reference root).  All
 * arrays are FP64, row-major, caller-owned; setters copy into device memory
 * owned by the context.  `ptr_kind` is XT_PTR_HOST or XT_PTR_DEVICE.
 * Every call returns 0 on success or a negative XT_ERR_* code; the message of
 * the last failure is available from xt_last_error().
 */
#ifndef XTDDFT_AMD_H
#define XTDDFT_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define XT_ABI_VERSION 8

#define XT_PTR_HOST 0
#define XT_PTR_DEVICE 1

/* operator kinds */
#define XT_KIND_XTDA 0     /* spin-adapted X-TDA on ROKS        (XTDA.py:558-692, self.X)   */
#define XT_KIND_UTDA 1     /* unrestricted TDA on UKS          (XTDA.py:685-687)            */
#define XT_KIND_SF_DOWN 2  /* spin-flip down  (SF_TDA.py:162-244, isf=-1)                   */
#define XT_KIND_SF_UP 3    /* spin-flip up    (SF_TDA.py:162-244, isf=+1)                   */
#define XT_KIND_XSF 4      /* spin-adapted spin-flip down (XSF_TDA.py:1029-1277)           */

/* exchange-correlation kernel types */
#define XT_XC_NONE 0       /* pure Hartree-Fock response (XTDA.py:546-554)                 */
#define XT_XC_LDA 1
#define XT_XC_GGA 2
#define XT_XC_MGGA 3       /* meta-GGA: (rho, grad rho, tau) kernel, XTDA.py:239-276 / nr_uks_fxc   */

/* spin-flip XC kernels (SF_DOWN / SF_UP / XSF; the reference's `method`) */
#define XT_SF_ALDA0 0      /* method 0: collinear-limit ALDA0, density only (SF_TDA.py:39-160)     */
#define XT_SF_MC 1         /* method 1: multicollinear kernel over (s, grad s[, tau_s])            */
                           /*   (_gen_uhf_tda_response_sf / nr_uks_fxc_sf_tda_mc, SF_TDA.py:855-1047) */

typedef struct xt_ctx xt_ctx;

typedef struct xt_desc {
  int kind;          /* XT_KIND_* */
  int restricted;    /* 1: ROKS (one MO basis), 0: UKS (alpha/beta bases) */
  int nao, nmo;
  int nc, no, nv;    /* closed / open / virtual counts (utils.get_cov, utils.py:6-41) */
  int naux;          /* DF functions held by THIS context (a shard when distributed) */
  int ngrid;         /* grid points held by THIS context */
  int xctype;        /* XT_XC_* */
  double hyb;        /* rsh_and_hybrid_coeff (XTDA.py:501) */
  double alpha;
  double omega;      /* != 0: long-range factor set with xt_set_jk_df(which=1) */
  double si;         /* spin/2 (XTDA.py:613); XSF uses no/2 (XSF_TDA.py:1061) */
  int sa;            /* XSF spin-adaptation level 0..3 (XSF_TDA.py:148-152) */
  double foo, fglobal; /* XSF scale factors (XSF_TDA.py:1501-1518) */
  int remove;        /* XSF: compress the OO block by one vector (XSF_TDA.py:397-414) */
  int add_local;     /* 1: add the rank-local one-electron terms (Fock, Delta-A Fock
                        parts); set on exactly one rank of a sharded operator */
  int device;        /* HIP device ordinal */
  int sf_kernel;     /* spin-flip kinds: XT_SF_ALDA0 or XT_SF_MC (ignored otherwise) */
} xt_desc;

/* lifetime ------------------------------------------------------------- */
int xt_create(const xt_desc* desc, xt_ctx** out);
int xt_destroy(xt_ctx* ctx);
int xt_set_stream(xt_ctx* ctx, void* hip_stream);
const char* xt_last_error(void);
int xt_abi_version(void);
/* SHA-256 prefix of the sources, headers and flags the library was built from
   (xtddft_amd/build.py source_hash); the Python loader refuses a library whose
   id differs from its tree. */
const char* xt_build_id(void);

/* one-time setup (what the reference builds once per solve) ------------ */
/* MO coefficients (nao x nmo); c_beta ignored when restricted.
   Replaces mf.mo_coeff consumption in _gen_tda_operation (XTDA.py:565-586). */
int xt_set_orbitals(xt_ctx* ctx, const double* c_alpha, const double* c_beta, int ptr_kind);
/* KS and pure-HF Fock matrices in the MO basis (nmo x nmo each), or the orbital
   energies for UTDA via xt_set_orbital_energies.
   Replaces mf.get_veff/get_hcore + scf.ROHF(mol).get_veff (XTDA.py:588-613,
   XSF_TDA.py:1070-1114). */
int xt_set_fock_mo(xt_ctx* ctx, const double* fa, const double* fb,
                   const double* fa_hf, const double* fb_hf, int ptr_kind);
int xt_set_orbital_energies(xt_ctx* ctx, const double* e_a, const double* e_b, int ptr_kind);
/* Density-fitting factor B[P,mu,nu] (naux x nao x nao) defining
   (mu nu|la si) = sum_P B B.  which = 0: full-range Coulomb, 1: long-range.
   Replaces mf.get_jk / get_j / get_k (XTDA.py:518-543, SF_TDA.py:273-281,
   XSF_TDA.py:996) -- the AO->MO transform is done once here on the device. */
int xt_set_jk_df(xt_ctx* ctx, const double* cderi, int which, int ptr_kind);
/* Stored 4-index ERIs instead of a DF factor (jk_mode ERI8): PySCF 8-fold
   packed order ('s8', ao2mo.restore(8, ...)): pair index ij = i(i+1)/2 + j
   (i >= j), npair = nao(nao+1)/2, (ij|kl) stored at ij(ij+1)/2 + kl (ij >= kl).
   Factorised on the device by pivoted Cholesky, (mu nu|la si) = sum_P L_P L_P,
   down to a largest residual diagonal <= tol (tol <= 0: 1e-13 x the largest
   diagonal), i.e. exact to that tolerance; the Cholesky vectors then drive the
   same MO-route J/K engine as xt_set_jk_df.  The context keeps the vectors of
   the contiguous block p_rank of p_count (multi-GPU aux sharding; 0, 1 for
   all) and takes that count as its naux (xt_naux); a long-range set (which = 1)
   of a different rank is zero-padded to a common naux.
   Replaces the incore mf._eri consumed by PySCF get_jk / get_k(omega=)
   (XTDA.py:518-543, SF_TDA.py:273-281, XSF_TDA.py:857,996). */
int xt_set_jk_eri8(xt_ctx* ctx, const double* eri_s8, int which, double tol,
                   int p_rank, int p_count, int ptr_kind);
/* DF / Cholesky functions held by this context (desc.naux, or the rank
   found by xt_set_jk_eri8) and the full Cholesky rank of the last
   xt_set_jk_eri8 (before sharding). */
int xt_naux(const xt_ctx* ctx, int* naux_local, int* chol_rank);
/* AO values on the grid (ncomp x ngrid x nao; ncomp = 1 LDA / 4 GGA and MGGA;
   spin-flip ALDA0: 1), weights (ngrid) and the kernel: UKS fxc (2 x nk x 2 x nk x ngrid,
   un-weighted; nk = 1 LDA, 4 GGA, 5 MGGA with tau = 1/2 sum |grad phi|^2 last) for
   XTDA/UTDA; for SF/XSF the weighted ALDA0 kernel (ngrid), or with XT_SF_MC the
   un-weighted multicollinear kernel fxc_sf (nk x nk x ngrid, the output of mcfun's
   eval_xc_eff_sf; the library applies the reference's factor 2 and the weights).
   Replaces ni.cache_xc_kernel / cache_xc_kernel_sf / cache_xc_kernel_sf_mc
   (XTDA.py:504, SF_TDA.py:39-88, 942-974) and the per-call grid loop of ni.nr_uks_fxc /
   nr_uks_fxc_sf_tda / nr_uks_fxc_sf_tda_mc (XTDA.py:514, SF_TDA.py:90-160, 976-1047). */
int xt_set_grid(xt_ctx* ctx, const double* ao, const double* weights,
                const double* kernel, int ptr_kind);
/* XTDA / UTDA only: the VV10 non-local correlation (NLC) term of the response, the
   v1 += get_vnlc_resp(mf, mol, mo_coeff, mo_occ, dm1[0] + dm1[1]) of XTDA.py:515-517.
   ao (4 x ngrid_nlc x nao: value, d/dx, d/dy, d/dz) on the NLC grid, its coordinates
   (ngrid_nlc x 3, Bohr) and weights, the VV10 parameters (b, C) and the density threshold
   rho_min (points with rho <= rho_min take no part).  Transforms the AOs to MO values,
   forms rho0 and grad rho0 from the occupied orbitals of both spins (xt_set_orbitals must
   have been called) and runs xt_vv10_ground once.  Afterwards xt_apply adds, per spin channel,
   C_occ^T V1 C_vir with V1 the second derivative of the VV10 energy (see xt_vv10_response)
   applied to the total first-order density; its time counts in the xc slot of
   xt_last_timings.  The NLC grid is independent of xt_set_grid's. */
int xt_set_nlc(xt_ctx* ctx, int ngrid_nlc, const double* ao, const double* coords,
               const double* weights, double b, double C, double rho_min, int ptr_kind);
/* XSF only: OO compression basis vects (no^2 x (no^2-1)) (XSF_TDA.py:397-414). */
int xt_set_oo_basis(xt_ctx* ctx, const double* vects, int ptr_kind);

/* exchange evaluation: the K part of get_jk / get_k (XTDA.py:518-543,
   SF_TDA.py:273-281, XSF_TDA.py:996).  XT_K_DIRECT contracts the MO DF factor
   per A.x (cost 2 naux nz O V^2); XT_K_STORED builds once per solve the MO
   exchange matrix Kx[(i,a),(j,b)] = sum_P B_P[i,j] B_P[a,b] (x the hybrid
   coefficients) and keeps it in HBM ((O V)^2 doubles per MO basis), making the
   per-A.x exchange one HBM-streaming GEMM -- PySCF's incore-vs-direct choice
   (mf._eri kept when it fits max_memory).  XT_K_AUTO (default) stores when
   the matrix fits max_gib (<= 0: free HBM minus a reserve).  The XSF Delta-A
   exchange blocks always run direct. */
#define XT_K_AUTO 0
#define XT_K_DIRECT 1
#define XT_K_STORED 2
int xt_set_exchange_mode(xt_ctx* ctx, int mode, double max_gib);
/* Build what is built once per solve (the stored exchange matrix when the
   mode resolves to it; xt_apply would otherwise build it on first use) and
   report the resolved mode and its HBM footprint (GiB).  A partitioned context
   (xt_set_partition with a proper aux window) that stores the exchange then drops
   the MO-factor rows outside its window (every later use reads only the window):
   xt_naux reports the window; re-partitioning or a stored-exchange rebuild needs
   the factor set again. */
int xt_prepare(xt_ctx* ctx, int* k_mode, double* k_gib);
/* What XT_K_AUTO resolves to on this context (*stored = 1 / 0) and the stored
   matrix's footprint (GiB; 0 for an operator without exchange), without building
   anything.  The resolution depends
   on this GPU's free HBM, so the ranks of a partitioned operator must agree
   before they build: a rank that streams its stored ROWS and a rank that
   contracts its aux WINDOW directly do not sum to the operator.  The host side
   takes the minimum over ranks and sets the mode explicitly
   (xtddft_amd/operator.py).  Same fit rule as xt_prepare. */
int xt_exchange_plan(xt_ctx* ctx, int* stored, double* k_gib);

/* Rank partition of a sharded operator (one process per GPU):
   the context keeps the whole MO factor but contracts J, the direct exchange
   and the XSF Delta-A only over aux rows [p0, p1), and stores / applies only
   the exchange rows whose occupied index is in [i0, i1) (superset O index).
   Over ranks with disjoint windows and row blocks the partial sigma sum to
   the full operator.  Defaults: all rows.  Call after the factor is set. */
int xt_set_partition(xt_ctx* ctx, int p0, int p1, int i0, int i1);

/* the hot path --------------------------------------------------------- */
/* sigma = A z for nz trial vectors, row-major (nz x dim) in the reference's
   vector order (PySCF order for XTDA/UTDA/SF; cv|co|ov|oo for XSF, OO
   compressed when remove).  Replaces the vind closures (XTDA.py:615-690,
   SF_TDA.py:224-243, XSF_TDA.py:1131-1276). */
int xt_apply(xt_ctx* ctx, int nz, const double* z, double* sigma, int ptr_kind);
int xt_dim(const xt_ctx* ctx);
/* per-phase device timings of the last xt_apply (ms): jk, xc, local, total */
int xt_last_timings(const xt_ctx* ctx, double* out4);

/* live timing of GEMM classes with HIP events on the context's stream (mask bit t:
   t = 1 exchange contraction (stored or direct), 2 XC forward U, 3 XC back L,
   4 XC forward W (fused rho), 5 XC back M (fused generated operand); 0 = off);
   xt_profile_stats(tag): {device ms summed over the launches of the last xt_apply,
   number of launches, algorithmic flops} */
int xt_set_profile(xt_ctx* ctx, int tag);
int xt_profile_stats(const xt_ctx* ctx, int tag, double* out3);
/* compulsory HBM bytes of class `tag` in the last xt_apply (each operand once) */
int xt_profile_bytes(const xt_ctx* ctx, int tag, double* bytes);

/* XSF preconditioner J diagonals (XSF_TDA.py:859-913): co_j (nc x no), ov_j (no x nv). */
int xt_xsf_j_diagonals(xt_ctx* ctx, double* co_j, double* ov_j, int ptr_kind);

/* device linear algebra used by the Davidson solver (Davidson.py:21-298) ---- */
/* C = alpha * op(A) op(B) + beta * C on device pointers (strided, batched);
   trans flags: 0 = as stored row-major, 1 = transposed. */
int xt_dgemm(int transa, int transb, int m, int n, int k, double alpha,
             const double* a, long lda, const double* b, long ldb, double beta,
             double* c, long ldc, void* hip_stream);
/* C[b] = alpha * sum_r A[b,r] B[b,r] + beta * C[b] with explicit strides: A(m, k) at
   a + b sAb + r sAr + m sAm + k sAk (sAm or sAk = 1), B(k, n) likewise (sBk or sBn = 1),
   C row-major with ldc, batch stride sCb.  The strided, reduce-indexed contraction the
   MO transforms and J/K builds run (lib.einsum over the DF index behind get_jk,
   XTDA.py:518-543); exposed so every engine layout is testable. */
int xt_dgemm_strided(int m, int n, int k, int r, int nbatch, double alpha,
                     const double* a, long sAm, long sAk, long sAr, long sAb,
                     const double* b, long sBk, long sBn, long sBr, long sBb, double beta,
                     double* c, long ldc, long sCb, void* hip_stream);
/* The engine behind xt_dgemm with every field of its contraction exposed, so that each tile
   configuration, staging path and layout it can launch is reachable from a test:
     C[b1,b2](m, n) = alpha sum_{r' < r} sum_{k' < k} A(b, r', m, k') B(b, r', k', n) + beta C[b1,b2](m, n)
     A(b, r', m, k') = a[b1 sAb1 + b2 sAb2 + r' sAr + m sAm + k' sAk]      (sAm or sAk = 1)
     B(b, r', k', n) = b[b1 sBb1 + b2 sBb2 + r' sBr + k' sBk + n sBn]      (sBk or sBn = 1)
     C[b1,b2](m, n)  = c[b1 sCb1 + b2 sCb2 + m ldc + n]
   rdiv > 0 (A m-contiguous only; the stored-exchange build's rows): row m = (hi, lo) =
   (m / rdiv, m % rdiv) sits at hi sAm_hi + lo in A and at hi sC_hi + lo ldc in C.
   max_split > 0 caps the split-K count; tag 0..5 selects a call site's kernel symbol and
   planning rule and must come with that site's layout (1, 4: A k-contiguous and B
   n-contiguous; 2: both k-contiguous; 3, 5: A m-contiguous and B n-contiguous).  Strides are
   >= 0 (0 broadcasts an operand over a batch index). */
typedef struct xt_gemm_desc {
  int m, n, k, r, nb1, nb2;
  double alpha, beta;
  long sAm, sAk, sAr, sAb1, sAb2;
  long sBk, sBn, sBr, sBb1, sBb2;
  long ldc, sCb1, sCb2;
  int rdiv; long sAm_hi, sC_hi;
  int max_split, tag;
  long ws_bytes;            /* split-K workspace cap; 0 = the default 256 MiB */
} xt_gemm_desc;
/* What xt_gemm_run would launch for this descriptor -- host only, no HIP call: the tile
   configuration (index, bm x bn tile, bk-deep K tiles), the split-K count after the
   workspace cap, and whether every K tile takes the masked staging (r > 1 and k % bk != 0).
   m = 0 or n = 0 launches nothing: cfg = -1, the rest 0. */
int xt_gemm_plan(const xt_gemm_desc* desc, int* cfg, int* bm, int* bn, int* bk, int* nsplit, int* masked);
/* Runs the contraction (plain mode, device pointers) on hip_stream.  The descriptor is
   validated before any HIP call. */
int xt_gemm_run(const xt_gemm_desc* desc, const double* a, const double* b, double* c, void* hip_stream);
/* y = (x - e*w) / clamp(d - (e - shift)) row-wise; diag preconditioner
   (XTDA.py:736-744, PySCF make_diag_precond). nrow vectors of length dim. */
int xt_precond(int nrow, int dim, const double* diag, const double* e, double shift,
               const double* r, double* out, void* hip_stream);
/* out[i] = sum_j x[i,j]^2 for nrow rows.  This and its two neighbours reject negative sizes
   and, where there is work, null pointers; nrow = 0 or dim = 0 returns 0 and touches nothing. */
int xt_row_norms2(int nrow, int dim, const double* x, double* out, void* hip_stream);
/* x[i,:] *= s[i] */
int xt_row_scale(int nrow, int dim, double* x, const double* s, void* hip_stream);

/* State-to-state transition moments of spin-flip amplitudes: out[x,i,j] =
   <state i| op_x |state j> for the roots of an XSF / SF-TDA solve (replaces the
   nstates^2 x 3 x 16 trace terms of XSF_TDA.calculate_TDM_R / calculate_TDM_U,
   XSF_TDA.py:435-592, and the moment loop of XSF_TDA_GPU.osc_str, XSF_TDA_GPU.py:936-1116).
   A state is the (nc+no) x (no+nv) amplitude matrix c (rows: occupied [c|o], columns:
   virtual [o|v]); with D_occ = c_occ^T op c_occ and D_vir = c_vir^T op c_vir the 16 terms
   are T[i,j] = sum c_i o (D c_j), D a symmetric linear map applied once per state:
     Y[c rows] = c[c rows] D_vir^(f1),  Y[o rows] = c[o rows] D_vir^(f2),
     Y[:, o cols] -= D_occ^(f2) c[:, o cols],  Y[:, v cols] -= D_occ^(f1) c[:, v cols],
     Y_co += f3 tr(oo) D_occ[c,o],  Y_ov -= f3 tr(oo) D_vir[o,v],
     Y_oo += f3 I (sum D_occ[c,o] o co - sum D_vir[o,v] o ov),
   M^(f) = M with its off-diagonal blocks (c<->o of D_occ, o<->v of D_vir) times f.
   sa = 0 (and every UKS reference): f = (1, 1, 0); otherwise, S = si (XSF_TDA.py:496-507),
   f1 = sqrt((2S+1)/2S), f2 = sqrt(2S/(2S-1)), f3 = 1/sqrt(2S(2S-1)).
   The AO->MO transforms, the pack of the vector rows into c, D for every component and
   state and the Gram contraction all run on the device inside the call; the products go
   through the engine behind xt_dgemm.  Reductions are fixed-order: two calls on the same
   input return the same bits.  The workspace lives for the call only; the part that grows
   with nstates is capped (768 MiB; states are processed in chunks). */
#define XT_TDM_LAYOUT_OV 0      /* a vector row is c itself, occ x vir row-major (PySCF's
                                   spin-flip order, SF_TDA.py:224-243) */
#define XT_TDM_LAYOUT_BLOCKS 1  /* the reference's cv|co|ov|oo blocks (XSF_TDA.py:509-515),
                                   OO compressed by vects when oo_compressed */
typedef struct xt_tdm_desc {
  int nao;
  int nc, no, nv;      /* c rows = nc + no, columns = no + nv (no = 0: SF-up, beta -> alpha) */
  int ncomp;           /* operator components (3 for a dipole) */
  int nstates;
  int sa;              /* 0: f = (1, 1, 0); != 0: the spin-adapted factors of si */
  double si;           /* S of the reference (mol.spin / 2) */
  int layout;          /* XT_TDM_LAYOUT_* */
  int oo_compressed;   /* block layout: the OO block holds no^2 - 1 coefficients of vects */
} xt_tdm_desc;
/* op_ao (ncomp, nao, nao) symmetric; c_occ (nao, nc+no); c_vir (nao, no+nv); vecs
   (nstates, dim) row-major; vects (no^2, no^2-1) or null; out (ncomp, nstates, nstates).
   All pointers of one ptr_kind. */
int xt_tdm(const xt_tdm_desc* desc, const double* op_ao, const double* c_occ, const double* c_vir,
           const double* vecs, const double* vects, double* out, int ptr_kind, void* hip_stream);

/* Transition moments between spin-conserving roots (X-TDA / U-TDA) and from the reference
   state to them: out[x,L,R] = <state L| op_x |state R> (replaces the nstates^2 calls of
   TDM_S and the nstates calls of TDM_GSS / TDM_SGS, x2c_hamiltonian/driver/tdm.py:6-126,
   that X_TDA.calculate_TDM loops over, xtddft/XTDA.py:1354-1400, and the host einsum of
   XTDA._transition).  A state is a row of vecs in the solver's own (PySCF) order [za | zb]:
   A = za (nocc_a x nvir_a), B = zb (nocc_b x nvir_b).  With d^a = C_a^T op C_a and
   d^b = C_b^T op C_b,
     T[L,R]  = tr(A_L d^a_vv A_R^T) - tr(A_L^T d^a_oo A_R)
             + tr(B_L d^b_vv B_R^T) - tr(B_L^T d^b_oo B_R)                  (all of U-TDA)
     T[0,R]  = T[R,0] = <d^a_ov, A_R> + <d^b_ov, B_R>,  T[0,0] = 0          (with_ground)
   and, for spin_adapted with no > 0 (ROKS: rows of A = [c|o], columns of B = [o|v]), in the
   spin-tensor basis of utils.so2st, cv1 = (A[c rows] - B[:, v columns]) / sqrt(2),
   co = B[:, o columns], ov = A[o rows]:
     T[L,R] -= h (sum co^L_iu d_ub cv1^R_ib + sum ov^L_ua d_ju cv1^R_ja) + (L <-> R),
     h = sqrt((S+1)/(2S)) - 1/sqrt(2),  d_ub = d^b_vv[o,v],  d_ju = d^a_oo[c,o].
   Phase: in so2st's phase the four couplings of CV(1) with CO(0) and OV(0) carry
   -sqrt((S+1)/(2S)); tdm.py:116-125 writes + because its CV(1) has the opposite sign.
   The form is bilinear, so Y_R = dT/dz_L is built once per state (engine GEMMs on the rows
   of vecs in place, small kernels for cv1 and its scatter) and one Gram product over dim
   gives every pair.  Reductions are fixed-order: two calls on the same input return the same
   bits.  The workspace lives for the call; the part that grows with nstates is capped
   (768 MiB, XT_TDM_WS_MIB lowers it; states are processed in chunks). */
typedef struct xt_tdm_sc_desc {
  int nao;
  int nocc_a, nvir_a, nocc_b, nvir_b;   /* za (nocc_a x nvir_a), zb (nocc_b x nvir_b) */
  int ncomp;          /* operator components (3 for a dipole) */
  int nstates;
  int spin_adapted;   /* 0: spin-orbital formula (U-TDA); 1: the X-TDA correction */
  int no;             /* spin_adapted: open shells; nocc_a - nocc_b = nvir_b - nvir_a = no */
  double si;          /* S of the reference, > 0 when spin_adapted and no > 0 */
  int with_ground;    /* 1: row / column 0 is the reference state */
} xt_tdm_sc_desc;
/* op_ao (ncomp, nao, nao) symmetric; c_occ_a (nao, nocc_a), c_vir_a (nao, nvir_a), c_occ_b
   (nao, nocc_b), c_vir_b (nao, nvir_b) (a block with no columns may be null); vecs (nstates,
   nocc_a nvir_a + nocc_b nvir_b) row-major; out (ncomp, n, n), n = nstates + with_ground.
   All pointers of one ptr_kind. */
int xt_tdm_sc(const xt_tdm_sc_desc* desc, const double* op_ao, const double* c_occ_a, const double* c_vir_a,
              const double* c_occ_b, const double* c_vir_b, const double* vecs, double* out, int ptr_kind,
              void* hip_stream);

/* Spin-orbit state interaction: the bilinear couplings of a real one-electron operator in the
   MO basis [c|o|v] between the roots of the three TDA manifolds of a high-spin ROKS reference
   and the reference state itself (SI_driver.make_hso_local / make_dm_local,
   x2c_hamiltonian/driver/si_driver.py:472-916; the 61 cases of si_driver.py:520-867 and the
   tables of x2c_hamiltonian/driver/tdm.py).  Groups in the order of the reference's H_eff,
   |S->, |GS>, |So>, |S+>; out[x][L][R], (ncomp, n, n), n = n_sm + with_ground + n_so + n_sp.
   State vectors in the reference's layouts, row-major blocks:
     |S->  [CV(1) nc x nv | CO(1) nc x no | OV(1) no x nv | O1O2 no x no | O1O1 no]
     |So>  [CV(0) nc x nv | CO(0) nc x no | OV(0) no x nv | CV(1) nc x nv]
     |S+>  CV(1) nc x nv
   XT_SI_SOC: op antisymmetric; the rank-1 tables interact_S_1S_1, _S_1GS, _S_1S, _GSS, _GSS1,
   _SS, _SS1, _S1S1 with hm replaced by the real component op[x] (every term is linear in hm
   with a real factor; the host forms h^m from the components).  Every same-manifold square
   block is filled in full, the other blocks with L before R in the group order; S-/S+, GS/GS
   and the blocks below the diagonal are zeros.  The CV(1) cases 45, 50, 54, 57, 59, 60 apply
   with S != 0 only.
   XT_SI_DIPOLE: op symmetric; the same-S blocks S-/S- (TDM_S_1), GS/So (TDM_GSS), So/So (TDM_S,
   with tdm.py's CV(1) phase: +sqrt((S+1)/(2S)), the opposite of utils.so2st) and S+/S+
   (TDM_S1); all else zeros.
   Arguments are validated before any HIP call (XT_ERR_ARG: negative counts, no state at all,
   s != no / 2, |S-> states with S < 1, a bad mode, with_ground or ptr_kind, null pointers
   where there is work, nmo or a vector length >= 2^21).  Every term is an engine GEMM on a
   block of op addressed in place by its strides; the O1O1 terms, the reference-state images
   and their placement are small kernels; one Gram product over the vector dimension per pair
   of groups.  No atomics, fixed-order reductions: two calls on the same input return the
   same bits.  The workspace lives for the call; the part that grows with the number of
   states is capped as in xt_tdm_sc (XT_TDM_WS_MIB; states are processed in chunks). */
#define XT_SI_SOC 0
#define XT_SI_DIPOLE 1
typedef struct xt_si_desc {
  int nc, no, nv;         /* nmo = nc + no + nv */
  int ncomp;              /* operator components (3) */
  double s;               /* S of the reference, = no / 2 */
  int n_sm, n_so, n_sp;   /* states of |S->, |So>, |S+> */
  int with_ground;        /* 1: the reference state is a group of one */
  int mode;               /* XT_SI_SOC / XT_SI_DIPOLE */
} xt_si_desc;
/* op_mo (ncomp, nmo, nmo); x_sm (n_sm, dim_sm), x_so (n_so, dim_so), x_sp (n_sp, nc nv)
   row-major (an empty group may be null); out (ncomp, n, n).  All pointers of one ptr_kind. */
int xt_si_couple(const xt_si_desc* desc, const double* op_mo, const double* x_sm, const double* x_so,
                 const double* x_sp, double* out, int ptr_kind, void* hip_stream);

/* VV10 non-local correlation on a quadrature grid: the pair sums behind the response term
   the reference takes from pyscf.hessian.rks.get_vnlc_resp (XTDA.py:515-517).  The energy is
     E = sum_i a_i [beta + 1/2 sum_j a_j Phi_ij],  a_i = w_i rho_i,  j = i included,
     Phi_ij = -3/2 / (g_ij g_ji (g_ij + g_ji)),  g_ij = omega0_i R_ij^2 + kappa_i,
     omega0 = sqrt(C gamma^2 / rho^4 + (4 pi / 3) rho),  gamma = |grad rho|^2,
     kappa = b (3/2) pi (9 pi)^(-1/6) rho^(1/6),  beta = (3 / b^2)^(3/4) / 32,
   over the points with rho > rho_min (a masked point is no source and receives zero).
   What is pinned is that the device term is the exact second derivative of this energy
   (tests/vv10_ref.py); parity with PySCF's get_vnlc_resp is not pinned.
   Device pointers; coords (ngrid x 3), weights, rho, gamma (ngrid); targets are the window
   [i0, i1), sources always all points.  Arguments are validated before any HIP call
   (negative sizes, i0 <= i1 <= ngrid, b > 0, C >= 0, rho_min >= 0, null pointers where there
   is work); an empty window (or nz = 0) returns 0 and touches nothing.  Reductions are
   fixed-order: two calls on the same input return the same bits.
   xt_vv10_ground: sums (6 x ngrid; the window's columns are written), with
   T_ij = a_j / (g_ij g_ji (g_ij + g_ji)), u_ij = 1/g_ij + 1/(g_ij + g_ji):
     F = -3/2 sum_j T_ij,  U = sum_j T_ij u_ij,  W = sum_j R_ij^2 T_ij u_ij,
     S0, S1, S2 = sum_j a_j Phi_xx {1, R_ij^2, R_ij^4}   (Phi_xx: second derivative in g_ij);
   dE/drho_i = w_i [beta + F + 3/2 rho_i (U dkappa/drho + W domega0/drho)],
   dE/dgamma_i = w_i 3/2 rho_i W domega0/dgamma. */
int xt_vv10_ground(int ngrid, const double* coords, const double* weights, const double* rho,
                   const double* gamma, double b, double C, double rho_min, int i0, int i1,
                   double* sums, void* hip_stream);
/* xt_vv10_response: (vrho1, vgamma1)[v, i] = sum_j d2E/d(rho, gamma)_i d(rho, gamma)_j applied
   to (rho1, gamma1)[v, j] for nz vectors, all four arrays (nz x ngrid) row-major; the window's
   columns of the outputs are written.  sums is xt_vv10_ground's output for the same data (at
   least over the window).  One kernel for every nz >= 1 and ngrid >= 1; a pair's kernel values
   are generated once per tile of up to 24 vectors. */
int xt_vv10_response(int ngrid, const double* coords, const double* weights, const double* rho,
                     const double* gamma, double b, double C, double rho_min, const double* sums,
                     int nz, const double* rho1, const double* gamma1, int i0, int i1,
                     double* vrho1, double* vgamma1, void* hip_stream);

/* Simplified open-shell TDA (sX-TDA / sU-TDA, xtddft/sTDA/os_sTDA.py) ------------------------
   Everything is in the active space: spin alpha has nocc_a = nc + no occupied and nvir_a = nv
   virtual orbitals, spin beta nocc_b = nc and nvir_b = no + nv.  A CSF is a triple (s, i, a):
   spin (0 alpha, 1 beta), occupied and virtual index in that spin's numbering; the classes are
   CV(aa) s = 0, i < nc; OV(aa) s = 0, i >= nc; CO(bb) s = 1, a < no; CV(bb) s = 1, a >= no.
   With the Loewdin charges q^A_pq = sum_{mu in A} C'_mu,p C'_mu,q (C' = S^1/2 C) and the
   Mataga-Nishimoto-Ohno-Klopman matrices gammaK, gammaJ (OSsTDA.gamma, os_sTDA.py:408-433)
     A[p,q] =  sum_AB q_ov[s_p][A,i_p,a_p] gammaK[A,B] q_ov[s_q][B,i_q,a_q]
             - d(s_p,s_q) sum_AB q_oo[s][A,i_p,i_q] gammaJ[A,B] q_vv[s][B,a_p,a_q]
             + d(s_p,s_q) (d(i_p,i_q) F_vv[s][a_p,a_q] - d(a_p,a_q) F_oo[s][i_p,i_q])
             + X(p,q)                                   (spin_adapted, no > 0, both CSFs of class CV)
             + d(p,q) delta_max / (1 + (K_pp / sigma_k)^4)                         (correct = 1)
   K_pp the first line at p = q.  X, with c1 = (1 - sqrt((S+1)/S) + 1/(2S))/2,
   c2 = (-1 + sqrt((S+1)/S) + 1/(2S))/2, c3 = 1/(4S), S = si, the ROHF-type Fock blocks H and the
   alpha virtual index a (beta: no + a): D_ab = H_b,vv[no+a,no+b] - H_a,vv[a,b],
   D_ij = H_b,oo[i,j] - H_a,oo[i,j];  CV(aa)-CV(aa): c1 d_ij D_ab + c2 d_ab D_ij;
   CV(bb)-CV(bb): c2 d_ij D_ab + c1 d_ab D_ij;  CV(aa)-CV(bb): c3 (d_ij D_ab + d_ab D_ij)
   (os_sTDA.py:263-325, 703-723).
   Numeric operands and outputs are device pointers in a pair-major layout (the natm charges of an
   orbital pair are contiguous); CSF lists and the atom AO offsets are HOST int arrays, so that
   every index is checked before the first HIP call (XT_ERR_ARG: negative sizes, an index outside
   its block, a null pointer where there is work, si <= 0 with spin_adapted and no > 0).  Empty
   work returns 0 and touches nothing.  Reductions are fixed-order: two calls on the same input
   return the same bits.
   Device and stream: the entries allocate on the CURRENT HIP device (the uploaded CSF lists and
   AO offsets; xt_stda_half's GEMM workspace), so the caller makes the device that owns the
   operands and hip_stream current before the call (hipSetDevice; torch.cuda.device).  Every
   call with work BLOCKS: it allocates, copies its host lists, launches on hip_stream,
   synchronises that stream and frees before it returns (xt_stda_half has no list: it queues
   engine GEMMs like xt_dgemm and may return before they finish).  The stream argument only orders the
   call against earlier work on that stream; a stream under graph capture cannot be used. */
typedef struct xt_stda_desc {
  int natm;
  int nocc_a, nvir_a, nocc_b, nvir_b;
  int nc, no, nv;       /* spin_adapted: nocc_a = nc + no, nvir_a = nv, nocc_b = nc, nvir_b = no + nv */
  int spin_adapted;     /* 1: the X term (ROKS) */
  double si;            /* S of the reference (mol.spin / 2) */
  int correct;          /* 1: the diagonal correction */
  double delta_max, sigma_k;
} xt_stda_desc;
/* device operands of the element generator, per spin (a spin no CSF uses may be null):
   q_ov, k_ov = gammaK q_ov  [(i nvir + a) natm + A];  q_oo [(i nocc + j) natm + A];
   j_vv = gammaJ q_vv [(a nvir + b) natm + A];  f_oo (nocc x nocc), f_vv (nvir x nvir) the KS Fock
   blocks;  h_oo, h_vv the ROHF-type Fock blocks (spin_adapted with no > 0 only). */
typedef struct xt_stda_ops {
  const double *q_ov_a, *k_ov_a, *q_oo_a, *j_vv_a, *f_oo_a, *f_vv_a, *h_oo_a, *h_vv_a;
  const double *q_ov_b, *k_ov_b, *q_oo_b, *j_vv_b, *f_oo_b, *f_vv_b, *h_oo_b, *h_vv_b;
} xt_stda_ops;
/* q_oo / q_ov / q_vv of one spin from cprime (nao x (nocc + nvir), occupied columns first, device)
   and the host offsets ao_off[natm + 1] of each atom's contiguous AOs (an atom may have one AO or
   none).  Replaces the per-atom einsum loop of os_sTDA.py:644-670. */
int xt_stda_charges(const xt_stda_desc* desc, int spin, int nao, const int* ao_off, const double* cprime,
                    double* q_oo, double* q_ov, double* q_vv, void* hip_stream);
/* k_ov = q_ov gammaK and j_vv = q_vv gammaJ of one spin (gamma symmetric natm x natm, device):
   engine GEMMs over the pair rows.  Replaces the gamma_k / gamma_j operands of every einsum in
   os_sTDA.py:33-44, 235-260, 263-325. */
int xt_stda_half(const xt_stda_desc* desc, int spin, const double* gamma_k, const double* gamma_j,
                 const double* q_ov, const double* q_vv, double* k_ov, double* j_vv, void* hip_stream);
/* e[p] = A[p,p] and kpp[p] = K_pp (kpp may be null) for a host list csf[3 n] of (s, i, a): the
   bits of xt_stda_matrix's diagonal on the same list.  Replaces iaia_f and the spin-adapted and
   correction additions, os_sTDA.py:33-44, 686-731. */
int xt_stda_diag(const xt_stda_desc* desc, const xt_stda_ops* ops, int n, const int* csf, double* e,
                 double* kpp, void* hip_stream);
/* w[q] = sum_{p in P} B[p,q]^2 / (e_n[q] - e_p[p] + 1e-10) for every q of the N list, B the first
   two lines of the generator; the P x N block is never stored.  Replaces the joblib loops over
   iajb_f, os_sTDA.py:235-260, 752-793. */
int xt_stda_select(const xt_stda_desc* desc, const xt_stda_ops* ops, int n_p, const int* csf_p,
                   const double* e_p, int n_n, const int* csf_n, const double* e_n, double* w, void* hip_stream);
/* The dense A (n x n, row-major, both triangles computed) of a CSF list in any order.  Replaces
   constractA and the block loops of os_sTDA.py:263-350, 1014-1221. */
int xt_stda_matrix(const xt_stda_desc* desc, const xt_stda_ops* ops, int n, const int* csf, double* a,
                   void* hip_stream);

/* mean-field front end ------------------------------ */
/* 3-index Coulomb integrals (ab|c) over contracted Cartesian Gaussians by
   McMurchie-Davidson (replaces libcint int3c2e behind PySCF df.incore.aux_e2,
   the DF factor whose get_jk XTDA.py:518-543 calls and whose MO transform
   stands in for ao2mo.general, XTDA.py:120).  Device pointers, launched on
   `hip_stream`; `out` is accumulated into (zero it first).
     pair_info[8k+0..5]  la, lb, npp, first row of pair_prim, offset in eab, first output row
     pair_prim[4q+0..3]  p, Px, Py, Pz of primitive pair q
     eab                 per pair [a][b][t][q]: Hermite coefficients x contraction coefficients
     aux_info[8j+0..5]   lc, nprim, first row of aux_prim, offset in ek, first output column, nc
     aux_prim[4r+0..3]   exponent, Cx, Cy, Cz
     ek                  per aux shell [c][u][r]: one-centre Hermite coefficients x coefficients
     out[(row0 + a*ncart(lb) + b) * ldo + col0 + c] += (ab|c)
   The ket may be a shell pair (4-index (ab|cd), the stored-ERI path of `jk_mode`
   ERI8 / PySCF mol.intor('int2e')): lc = l_c + l_d, nc = ncart(l_c) ncart(l_d),
   its primitive pairs in aux_prim and its pair Hermite coefficients in ek.
   lmax_orb <= 3 (f), 2 lmax_orb + lmax_aux <= 13 (lmax_aux: the ket's Hermite order).
   omega > 0: the long-range operator erf(omega r12)/r12 (PySCF mol.with_range_coulomb,
   the cderi_lr / eri_lr factors of range-separated hybrids, XTDA.py:501,527-539); 0: 1/r12. */
int xt_int3c2e_cart(int npair, const int* pair_info, const double* pair_prim, const double* eab,
                    int naux_shells, const int* aux_info, const double* aux_prim, const double* ek,
                    int lmax_orb, int lmax_aux, double omega, double* out, long ldo, void* hip_stream);
/* The same integrals with Schwarz screening and a diagonal mode -- the exact ERIs of
   the direct-SCF mean field (PySCF's default mf, whose get_jk XTDA.py:518-543 calls
   and whose ERIs ao2mo.general transforms, XTDA.py:120) without the 4-index array:
   the integral-direct pivoted Cholesky of xtddft_amd/qc/dchol.py evaluates the
   diagonal (ab|ab) (diag = 1: one block per bra pair with ket = the same table
   entry, nket == npair) and the pivot columns (all pairs | chosen pairs) through it.
   q_bra / q_ket (device, per table entry; both or neither): blocks with
   q_bra[k] q_ket[j] < q_thr are skipped (left zero).
   lmax_orb and lket size the kernel's private arrays (the bucket 2 lmax_orb <= 4 and
   2 lmax_orb + lket <= 8, or the full one).  The tables are device memory, so the
   per-entry values are not checked; every entry must satisfy the declared bounds:
   la, lb <= lmax_orb in every pair_info row and lc <= lket in every ket_info row.  An
   entry above them overruns those arrays.  Declaring more than the tables hold is
   allowed and gives the same bits. */
int xt_int2e_cart(int npair, const int* pair_info, const double* pair_prim, const double* eab,
                  int nket, const int* ket_info, const double* ket_prim, const double* ek,
                  int lmax_orb, int lket, double omega, const double* q_bra, const double* q_ket,
                  double q_thr, int diag, double* out, long ldo, void* hip_stream);
/* Coulomb integrals between charge distributions given directly as Hermite expansions: the
   derivative integrals of the spin-orbit mean field (the reference's sfX2C_soDKH1.py get_kint,
   get_wso and int1e_pnucp; xtddft_amd/qc/ints.py deriv_tables builds the tables).  As
   xt_int2e_cart, but every table entry states its Hermite order and its number of rows:
     bra_info[8k+0..6]   order, nrow, npp, first row of bra_prim, offset in eb, first output row, tag
     bra_prim[4q+0..3]   p, Px, Py, Pz of primitive pair q
     eb                  per entry [row][t][q] over nrow x ntuv(order) x npp
     ket_info[8j+0..6]   order, nprim, first row of ket_prim, offset in ek, first output column, ncol, tag
     ket_prim[4r+0..3]   exponent, Cx, Cy, Cz
     ek                  per entry [col][u][r] over ncol x ntuv(order) x nprim
   cross = 0: out[(row0 + row) * ldo + col0 + col] += (row|col).
   cross = 1: rows are (m, ab) and columns (n, cd) with m, n = x, y, z outermost (nrow = 3 nab,
   ncol = 3 ncd; row0 / col0 count ab / cd); the three cross products are written directly,
     out[(l * nrow_tot + row0 + ab) * ldo + col0 + cd] += eps_lmn ((m, ab)|(n, cd)),
   and the m = n products are never formed.  `out` is accumulated into (zero it first); blocks
   of different (bra, ket) entries must not overlap.  A (bra, ket) pair whose tags differ is
   skipped (the one-centre approximation: tag = atom; 0 everywhere computes every pair).  lbra / lket bound the orders of the two
   tables: lbra <= 8, lbra + lket <= 14.  The tables are device memory and are not read on the
   host; an entry whose order exceeds the declared bounds is skipped (its block stays zero). */
int xt_hint_cart(int nbra, const int* bra_info, const double* bra_prim, const double* eb,
                 int nket, const int* ket_info, const double* ket_prim, const double* ek,
                 int lbra, int lket, int cross, long nrow_tot, double* out, long ldo, void* hip_stream);
/* First-derivative Coulomb integrals contracted with a two-particle density to a force on the
   atoms: the two-electron part of an analytic nuclear gradient (the reference's
   grad_jp/grad/usfcis.py get_jk / get_k terms; xtddft_amd/qc/grad.py builds the tables),
     out[3A + m] += sum_{a on A} sum_{b,c,d} (d_m a  b|c d) Gamma_abcd,   m = x, y, z,
     Gamma_abcd = sum_{t < nterm} wj[t] P_t[a,b] Q_t[c,d] + wk[t] P_t[a,c] Q_t[b,d],
   d_m a being what the bra table holds for row (m, ca, cb): ints.py deriv_tables stores the
   derivative with respect to the centre of a, 2 alpha g_{l+1_m} - l_m g_{l-1_m}, the negative of
   the electron-coordinate derivative (the caller fixes the sign).  The integrals are
   xt_hint_cart's and are consumed where they are formed; nothing of size pairs x pairs is written.
     bra_info / bra_prim / eb   ordered pairs with the first function differentiated, as
                                xt_hint_cart's bra: order la + lb + 1, rows (m, ca, cb), nrow = 3 nab
     bra_ao[4k+0..3]            first Cartesian AO of a, of b, ncart(b), atom of a
     ket_info / ket_prim / ek   plain shell pairs c >= d, as xt_hint_cart's ket (ncol = ncd)
     ket_ao[4j+0..3]            first Cartesian AO of c, of d, ncart(d), 1 when c != d (the thread
                                then adds the (d, c) image of Gamma)
     wj, wk                     nterm host doubles each, 1 <= nterm <= 8
     p, q                       device, nterm matrices nao x nao each over Cartesian components,
                                row-major, not necessarily symmetric
   A thread owns one bra entry and at most `strip` ket entries (every nstrip-th one, nstrip =
   ceil(nket / strip)); the strips and then the bra
   entries of an atom are summed in table order by two small kernels, without atomics: equal
   inputs give equal bits.  `work` (device) holds at least 3 nbra (ceil(nket / strip) + 1) doubles,
   nwork states its length.  `out` (device, 3 natm) is accumulated into.  lbra / lket bound the
   orders as in xt_hint_cart (lbra <= 8, lbra + lket <= 14); an entry above them adds nothing. */
int xt_grad_jk(int nbra, const int* bra_info, const double* bra_prim, const double* eb, const int* bra_ao,
               int nket, const int* ket_info, const double* ket_prim, const double* ek, const int* ket_ao,
               int lbra, int lket, int nterm, const double* wj, const double* wk, const double* p,
               const double* q, long nao, int strip, int natm, double* work, long nwork, double* out,
               void* hip_stream);
/* xt_grad_jk with a Coulomb list and an exchange list of their own,
     Gamma_abcd = sum_{t < nj} wj[t] PJ_t[a,b] QJ_t[c,d] + sum_{t < nk} wk[t] PK_t[a,c] QK_t[b,d],
   for two-particle densities of more than eight pairs whose pairs are Coulomb-only or exchange-only
   (the U-TDA gradient on a hybrid: three Coulomb and eight exchange pairs): one pass over the
   derivative integrals, and one product per pair where xt_grad_jk forms two.  The integral code, the
   (d, c) image, the Gamma cache, the strips and the two-stage reduction are xt_grad_jk's own (one
   kernel body, instantiated for either Gamma); tables, strip, work / nwork, out, lbra / lket as there.
     wj, pj, qj    nj host weights; device, nj matrices nao x nao each (as p, q of xt_grad_jk)
     wk, pk, qk    nk host weights; device, nk matrices each
   0 <= nj <= 8, 0 <= nk <= 8, nj + nk >= 1.  A list whose count is zero is not read: its three
   pointers may be null.  Equal inputs give equal bits. */
int xt_grad_jk2(int nbra, const int* bra_info, const double* bra_prim, const double* eb, const int* bra_ao,
                int nket, const int* ket_info, const double* ket_prim, const double* ek, const int* ket_ao,
                int lbra, int lket, int nj, const double* wj, const double* pj, const double* qj, int nk,
                const double* wk, const double* pk, const double* qk, long nao, int strip, int natm,
                double* work, long nwork, double* out, void* hip_stream);
/* xt_grad_jk2 with the derivative integrals (d_m a b|c d) taken over erf(omega r12) / r12, the long-range
   operator of a range-separated hybrid (CAM-B3LYP, wB97X-D): the same Gamma over the same tables.  Per
   primitive quartet with alpha = p s / (p + s) the Hermite integrals are those of
   a2 = alpha omega^2 / (alpha + omega^2) times sqrt(a2 / alpha), the formula of xt_int2e_cart; the Boys
   table, the image, the Gamma cache, the strips and the reduction are xt_grad_jk2's (one kernel body,
   the operator a compile-time parameter).  The exchange of such a functional is
   hyb K + (alpha - hyb) K_LR, so its gradient is two calls: xt_grad_jk2 with the Coulomb list and the
   exchange list weighted by hyb, and xt_grad_jk2_lr with nj = 0 and the same exchange pairs weighted
   by alpha - hyb.  Arguments, limits and errors as xt_grad_jk2; omega must be finite and > 0 (1/r12
   is xt_grad_jk2).  Equal inputs give equal bits. */
int xt_grad_jk2_lr(int nbra, const int* bra_info, const double* bra_prim, const double* eb, const int* bra_ao,
                   int nket, const int* ket_info, const double* ket_prim, const double* ek, const int* ket_ao,
                   int lbra, int lket, int nj, const double* wj, const double* pj, const double* qj, int nk,
                   const double* wk, const double* pk, const double* qk, long nao, int strip, int natm,
                   double* work, long nwork, double* out, void* hip_stream, double omega);
/* AO values (deriv 0) or values and gradients (deriv 1) of normalised spherical
   AOs on grid points (PySCF mol.eval_ao / ni.block_loop, SF_TDA.py:63-68, the AO
   input of cache_xc_kernel / nr_uks_fxc, XTDA.py:504,514), device pointers:
     coords[3g + 0..2]      grid point (Bohr)
     shell_info[8s + 0..3]  l (<= 4), nprim, offset in shell_data, first AO
     shell_data[off ..]     nprim exponents, nprim coefficients (x radial norms), centre
     sph                    solid-harmonic tables of l = 0..4 ((2l+1) x ncart(l) each,
                            concatenated, libcint order)
     ao_norm[ao]            AO normalisation
     out[c * comp_stride + g * ldo + ao], c = value (, d/dx, d/dy, d/dz). */
int xt_eval_ao(int ngrid, const double* coords, int nshell, const int* shell_info,
               const double* shell_data, const double* sph, const double* ao_norm, int deriv,
               double* out, long ldo, long comp_stride, void* hip_stream);
/* The exchange-correlation force on the atoms at fixed spin density matrices: the nuclear
   derivative of the XC potential matrix contracted with the ground-state density (PySCF
   grad.uks.get_vxc, the vxc1[:, 1:] the reference's grad_hb/tduks_sfu.py:168-177 adds to the
   mean-field gradient; xtddft_amd/qc/grad.py grad_xc_device), without grid-weight derivatives:
     out[3A + x] += sum_{s < nspin} sum_{g < ngrid} sum_{mu on A}
                      d_x phi_mu(g) e_s(g, mu) + (sum_{k = x,y,z} h_s(k, g) d_x d_k phi_mu(g)) c_s(g, mu)
   (the caller applies the factor -2).  The AO first and second derivatives are evaluated where
   they are consumed; no derivative plane is written.  Device pointers:
     coords, shell_info, shell_data, sph, ao_norm   as xt_eval_ao (l <= 4)
     shell_atom[s]      the atom (row of out) of shell s; shells of one atom need not be adjacent
     lmax               bound of l over the shell table, 0 <= lmax <= 4; a shell above it, or one
                        whose AO range leaves [0, nao), adds nothing
     xctype             XT_XC_LDA: the first term only -- h and c are not read and may be null;
                        XT_XC_GGA: both terms
     h[(4 s + k) ldg + g]       k = 1..3: w_g d eps / d(d_k rho_s), the "eff" layout of the XC
                                derivatives without any halving; plane k = 0 (d eps / d rho_s) is
                                part of e and is never read
     e[(s nao + mu) ldg + g]    e_s = b_s D_s with b_s = h_s(0) phi + sum_k h_s(k) d_k phi
     c[(s nao + mu) ldg + g]    c_s = phi D_s
   e and c are AO-major ([ao][g], ldg >= ngrid doubles between AOs) so that the lanes of a wave,
   which are 64 consecutive grid points of one shell, read consecutive doubles; the GEMM engine
   gives that layout as D_s b_s^T.  Reduction without atomics: a block (one shell x a tile of 64
   grid points in GGA mode, where its four waves share out the four weights of the bracket, of
   256 points in LDA mode) writes one partial sum; the grid tiles of a shell and then the shells
   of an atom are summed in ascending order by two small kernels, so equal inputs give equal
   bits.  `work` (device) holds at least 3 nshell (ceil(ngrid / 64) + 1) doubles in either mode,
   nwork states its length.  `out` (device, 3 natm) is accumulated into.  XT_ERR_ARG before any
   launch: negative sizes, ldg < ngrid, lmax outside 0..4, nspin not 1 or 2, xctype not LDA /
   GGA, nwork too small, more than 2^31 blocks, a null pointer that would be read. */
int xt_grad_xc(int ngrid, const double* coords, int nshell, const int* shell_info,
               const double* shell_data, const double* sph, const double* ao_norm,
               const int* shell_atom, int lmax, int natm, int nao, int nspin, int xctype,
               const double* h, const double* e, const double* c, long ldg, double* work, long nwork,
               double* out, void* hip_stream);
/* The exchange-correlation linear response of a UKS reference in the AO route, everything that is
   not a GEMM (xtddft_amd/qc/device.py DeviceEngine.fxc_response: the XC part of the UKS
   gen_response(hermi=1) of the Z-vector equations and the f^xc[T] of the spin-flip TDA gradient).
   For symmetric trial densities dm_s, with c_s = phi dm_s formed by the caller (one GEMM per spin):
     rho1_s(0, g) = sum_mu phi_mu(g) c_s(g, mu),   rho1_s(k, g) = 2 sum_mu d_k phi_mu(g) c_s(g, mu)
     wv_s(k, g)   = w_g sum_{s' k'} fxc(s, k, s', k', g) rho1_s'(k', g)       ("eff" layout, nothing halved)
     b_s(g, mu)   = 1/2 wv_s(0, g) phi_mu(g) + sum_k wv_s(k, g) d_k phi_mu(g)  (XT_XC_GGA)
     b_s(g, mu)   = wv_s(0, g) phi_mu(g)                                       (XT_XC_LDA)
   so that V^resp_s = phi^T b_s (GGA: plus its transpose).  Device pointers, ncomp = 1 (LDA) or 4 (GGA):
     ao[k ao_plane + g ldao + mu]    k = 0 (value) or 0..3 (value, d/dx, d/dy, d/dz); LDA reads plane 0 only
     c[(s ngrid + g) ldc + mu]       c_s = phi dm_s
     fxc[((s ncomp + k) 2 ncomp + s' ncomp + k') ldg + g]   as eval_xc_eff returns it, g innermost
     w[g]                            grid weights
     rho1[(4 s + k) ldo + g], wv[(4 s + k) ldo + g]   outputs; LDA writes plane k = 0 only
     b[(s ngrid + g) ldb + mu]       output
   Any of rho1, wv, b may be null: that output is skipped (all three null: nothing is launched).  A
   block owns 64 consecutive grid points; no atomics, the summation order is fixed and does not depend
   on the alignment of the operands, so equal inputs give equal bits.  A point whose fxc entries are
   all zero gets wv = 0 and b = 0 provided c is finite there.  ngrid = 0 or nao = 0 returns 0 without
   a launch.  XT_ERR_ARG before any HIP call: negative sizes, ldao / ldc / ldb < nao, ldg / ldo <
   ngrid, ao_plane shorter than one plane's rows (GGA), xctype not LDA / GGA, more than 2^31 blocks,
   a null ao, c, fxc or w. */
int xt_xc_resp(long ngrid, int nao, int xctype, const double* ao, long ao_plane, long ldao,
               const double* c, long ldc, const double* fxc, long ldg, const double* w,
               double* rho1, double* wv, long ldo, double* b, long ldb, void* hip_stream);
/* The spin-flip channel of the multicollinear kernel in the AO route (DeviceEngine.fxc_sf_response:
   the f^xc_sf[X] potential and weights of the multicollinear spin-flip TDA gradient).  One channel;
   with c = phi X_S formed by the caller, X_S the symmetrised transition density:
     rho1(0, g) = sum_mu phi_mu(g) c(g, mu),   rho1(k, g) = 2 sum_mu d_k phi_mu(g) c(g, mu)
     wv(k, g)   = 2 w_g sum_k' fxc_sf(k, k', g) rho1(k', g)                   (nothing halved)
     b(g, mu)   = 1/2 wv(0, g) phi_mu(g) + sum_k wv(k, g) d_k phi_mu(g)       (XT_XC_GGA)
     b(g, mu)   = wv(0, g) phi_mu(g)                                          (XT_XC_LDA)
   Device pointers, nk = 1 (LDA) or 4 (GGA):
     ao[k ao_plane + g ldao + mu], w[g]   as for xt_xc_resp
     c[g ldc + mu]                        c = phi X_S
     fxc_sf[(k nk + k') ldg + g]          the multicollinear kernel (mcol.sf_mc_kernel), g innermost
     rho1[k ldo + g], wv[k ldo + g]       outputs; LDA writes plane 0 only
     b[g ldb + mu]                        output
   Any of rho1, wv, b may be null (all three: nothing is launched).  Blocks, summation order, zero
   weights, zero sizes and the XT_ERR_ARG list are those of xt_xc_resp. */
int xt_xc_resp_sf(long ngrid, int nao, int xctype, const double* ao, long ao_plane, long ldao,
                  const double* c, long ldc, const double* fxc_sf, long ldg, const double* w,
                  double* rho1, double* wv, long ldo, double* b, long ldb, void* hip_stream);
/* The rows b_ch of given grid weights, nch = 1..4 channels with the AO rows read once for all:
     b[(ch ngrid + g) ldb + mu] = 1/2 wv(ch, 0, g) phi_mu(g) + sum_k wv(ch, k, g) d_k phi_mu(g)   (XT_XC_GGA)
     b[(ch ngrid + g) ldb + mu] = wv(ch, 0, g) phi_mu(g)                                          (XT_XC_LDA)
   with wv[(4 ch + k) ldo + g] (LDA reads plane k = 0 only), so that the potential of the weights is
   phi^T b_ch (GGA: plus its transpose).  The arithmetic is the third pass of xt_xc_resp: on the wv
   that call wrote, nch = 2 gives its b bit for bit.  A null b returns 0 without a launch.  XT_ERR_ARG
   before any HIP call: negative sizes, nch outside 1..4, ldao / ldb < nao, ldo < ngrid, ao_plane
   shorter than one plane's rows (GGA), xctype not LDA / GGA, more than 2^31 blocks, a null ao or wv. */
int xt_xc_rows(long ngrid, int nao, int xctype, int nch, const double* ao, long ao_plane, long ldao,
               const double* wv, long ldo, double* b, long ldb, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
