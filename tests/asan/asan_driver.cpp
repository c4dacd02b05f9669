// Host-side AddressSanitizer check of the C ABI (include/xtddft_amd.h), built with
// tools/asan_host.sh (every csrc/*.hip with -Xarch_host -fsanitize=address).  Runs on a
// machine without a GPU: it drives the argument validation and error-reporting paths of
// the entry points -- every rejected call must return a negative code and leave a
// readable message in xt_last_error -- under ASan (heap / stack / global overflows,
// use-after-free in the error-string handling and descriptor checks).
#include <cstdio>
#include <cstring>
#include "../../include/xtddft_amd.h"

static int failures = 0;
static void expect_err(int rc, const char* what) {
  const char* msg = xt_last_error();
  if (rc >= 0 || msg == nullptr || std::strlen(msg) == 0) {
    std::printf("FAIL %s: rc %d msg '%s'\n", what, rc, msg ? msg : "(null)");
    ++failures;
  }
}

int main() {
  if (xt_abi_version() <= 0) { std::printf("FAIL abi\n"); return 1; }
  if (!xt_build_id() || std::strlen(xt_build_id()) == 0) { std::printf("FAIL build id\n"); return 1; }
  xt_ctx* h = nullptr;
  expect_err(xt_create(nullptr, &h), "create null desc");
  xt_desc d;
  std::memset(&d, 0, sizeof(d));
  expect_err(xt_create(&d, &h), "create empty desc");
  d.kind = XT_KIND_XTDA; d.restricted = 1; d.nao = 10; d.nmo = 10; d.nc = 3; d.no = 2; d.nv = 4;
  expect_err(xt_create(&d, &h), "create nc+no+nv != nmo");
  d.nv = 5; d.si = 0.0;
  expect_err(xt_create(&d, &h), "create XTDA with zero spin");
  d.si = 1.0; d.restricted = 0;
  expect_err(xt_create(&d, &h), "create XTDA on UKS");
  d.kind = 99;
  expect_err(xt_create(&d, &h), "create unknown kind");
  d.kind = XT_KIND_XSF; d.restricted = 1; d.sa = 2; d.no = 1; d.nc = 4;
  expect_err(xt_create(&d, &h), "create XSF SA>0 with one open shell");
  d.kind = XT_KIND_XTDA; d.sa = 0; d.xctype = 17;
  expect_err(xt_create(&d, &h), "create bad xctype");
  d.kind = XT_KIND_SF_DOWN; d.xctype = XT_XC_GGA; d.no = 2; d.nc = 3; d.sf_kernel = 5;
  expect_err(xt_create(&d, &h), "create bad sf_kernel");
  d.sf_kernel = XT_SF_ALDA0;
  // null-context calls of every setter / query
  double buf[8] = {0};
  expect_err(xt_set_orbitals(nullptr, buf, buf, XT_PTR_HOST), "set_orbitals null");
  expect_err(xt_set_fock_mo(nullptr, buf, buf, buf, buf, XT_PTR_HOST), "set_fock_mo null");
  expect_err(xt_set_jk_df(nullptr, buf, 0, XT_PTR_HOST), "set_jk_df null");
  expect_err(xt_set_grid(nullptr, buf, buf, buf, XT_PTR_HOST), "set_grid null");
  expect_err(xt_apply(nullptr, 1, buf, buf, XT_PTR_HOST), "apply null");
  expect_err(xt_set_exchange_mode(nullptr, XT_K_AUTO, 0.0), "exchange_mode null");
  expect_err(xt_exchange_plan(nullptr, nullptr, nullptr), "exchange_plan null");
  expect_err(xt_set_profile(nullptr, 1), "profile null");
  expect_err(xt_profile_stats(nullptr, 1, buf), "profile_stats null");
  expect_err(xt_profile_bytes(nullptr, 9, buf), "profile_bytes bad tag");
  // device kernels: argument checks run before any HIP call
  expect_err(xt_dgemm_strided(-1, 4, 4, 1, 1, 1.0, buf, 1, 4, 0, 0, buf, 4, 1, 0, 0, 0.0, buf, 4, 0, nullptr),
             "dgemm_strided negative m");
  expect_err(xt_dgemm_strided(4, 4, 4, 1, 1, 1.0, buf, 2, 4, 0, 0, buf, 4, 1, 0, 0, 0.0, buf, 4, 0, nullptr),
             "dgemm_strided A without a unit stride");
  expect_err(xt_dgemm_strided(4, 4, 4, 1, 1, 1.0, buf, 4, 1, 0, 0, buf, 4, 1, 0, 0, 0.0, buf, 3, 0, nullptr),
             "dgemm_strided ldc < n");
  expect_err(xt_dgemm_strided(4, 4, 4, 1, 1, 1.0, nullptr, 4, 1, 0, 0, buf, 4, 1, 0, 0, 0.0, buf, 4, 0, nullptr),
             "dgemm_strided null A");
  expect_err(xt_dgemm_strided(4, 4, 4, 2, 1, 1.0, buf, 4, 1, -16, 0, buf, 4, 1, 16, 0, 0.0, buf, 4, 0, nullptr),
             "dgemm_strided negative stride");
  expect_err(xt_dgemm(0, 0, -1, 4, 4, 1.0, buf, 4, buf, 4, 0.0, buf, 4, nullptr), "dgemm negative m");
  expect_err(xt_dgemm(0, 0, 2, 2, 4, 1.0, buf, 3, buf, 2, 0.0, buf, 2, nullptr), "dgemm lda < k");
  expect_err(xt_dgemm(1, 0, 2, 2, 2, 1.0, buf, 1, buf, 2, 0.0, buf, 2, nullptr), "dgemm lda < m (transposed)");
  expect_err(xt_dgemm(0, 0, 2, 2, 2, 1.0, buf, 2, buf, 1, 0.0, buf, 2, nullptr), "dgemm ldb < n");
  expect_err(xt_dgemm(0, 1, 2, 2, 4, 1.0, buf, 4, buf, 3, 0.0, buf, 2, nullptr), "dgemm ldb < k (transposed)");
  expect_err(xt_dgemm(0, 0, 2, 2, 2, 1.0, buf, 2, buf, 2, 0.0, buf, 1, nullptr), "dgemm ldc < n");
  expect_err(xt_dgemm(0, 0, 2, 2, 2, 1.0, nullptr, 2, buf, 2, 0.0, buf, 2, nullptr), "dgemm null A");
  expect_err(xt_dgemm(0, 0, 2, 2, 0, 1.0, nullptr, 2, nullptr, 2, 0.0, nullptr, 2, nullptr), "dgemm null C");
  if (xt_dgemm(0, 0, 0, 2, 2, 1.0, nullptr, 2, nullptr, 2, 0.0, nullptr, 2, nullptr) != 0) {
    std::printf("FAIL dgemm m = 0 is a no-op\n"); ++failures;
  }
  expect_err(xt_precond(-1, 2, buf, buf, 0.0, buf, buf, nullptr), "precond negative nrow");
  expect_err(xt_precond(2, 2, buf, nullptr, 0.0, buf, buf, nullptr), "precond null e");
  expect_err(xt_precond(2, 2, buf, buf, 0.0, buf, nullptr, nullptr), "precond null out");
  expect_err(xt_row_norms2(2, -2, buf, buf, nullptr), "row_norms2 negative dim");
  expect_err(xt_row_norms2(2, 2, nullptr, buf, nullptr), "row_norms2 null x");
  expect_err(xt_row_scale(-2, 2, buf, buf, nullptr), "row_scale negative nrow");
  expect_err(xt_row_scale(2, 2, buf, nullptr, nullptr), "row_scale null s");
  buf[0] = 3.0;
  if (xt_precond(0, 2, buf, buf, 0.0, buf, buf, nullptr) != 0 || xt_row_norms2(2, 0, buf, buf, nullptr) != 0 ||
      xt_row_scale(0, 0, buf, buf, nullptr) != 0 || buf[0] != 3.0) {
    std::printf("FAIL zero-size helper calls are no-ops\n"); ++failures;
  }
  buf[0] = 0.0;
  {
    xt_gemm_desc g;
    std::memset(&g, 0, sizeof(g));
    int o[6];
    g.m = 4; g.n = 4; g.k = 4; g.r = 1; g.nb1 = 1; g.nb2 = 1; g.alpha = 1.0;
    g.sAm = 4; g.sAk = 1; g.sBk = 4; g.sBn = 1; g.ldc = 4;
    if (xt_gemm_plan(&g, o, o + 1, o + 2, o + 3, o + 4, o + 5) != 0 || o[0] != 4 || o[1] != 64 || o[4] != 1) {
      std::printf("FAIL gemm_plan of a valid descriptor\n"); ++failures;
    }
    expect_err(xt_gemm_plan(nullptr, o, o + 1, o + 2, o + 3, o + 4, o + 5), "gemm_plan null desc");
    expect_err(xt_gemm_plan(&g, nullptr, o + 1, o + 2, o + 3, o + 4, o + 5), "gemm_plan null output");
    expect_err(xt_gemm_run(&g, nullptr, buf, buf, nullptr), "gemm_run null A");
    g.ldc = 3;
    expect_err(xt_gemm_run(&g, buf, buf, buf, nullptr), "gemm_run ldc < n");
    g.ldc = 4; g.sAk = 2;
    expect_err(xt_gemm_plan(&g, o, o + 1, o + 2, o + 3, o + 4, o + 5), "gemm_plan A without a unit stride");
    g.sAk = 1; g.tag = 3;
    expect_err(xt_gemm_run(&g, buf, buf, buf, nullptr), "gemm_run tag 3 on (k, n) operands");
    g.tag = 0; g.rdiv = 2;
    expect_err(xt_gemm_plan(&g, o, o + 1, o + 2, o + 3, o + 4, o + 5), "gemm_plan rdiv with A k-contiguous");
    g.rdiv = 0; g.sBb2 = -1;
    expect_err(xt_gemm_run(&g, buf, buf, buf, nullptr), "gemm_run negative stride");
    g.sBb2 = 0; g.r = 0;
    expect_err(xt_gemm_plan(&g, o, o + 1, o + 2, o + 3, o + 4, o + 5), "gemm_plan r < 1");
  }
  expect_err(xt_int2e_cart(-1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, 0.0, nullptr,
                           nullptr, 0.0, 0, nullptr, 0, nullptr), "int2e negative npair");
  expect_err(xt_int2e_cart(1, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, 4, 0, 0.0, nullptr,
                           nullptr, 0.0, 0, nullptr, 0, nullptr), "int2e orbital l > 3");
  expect_err(xt_eval_ao(10, nullptr, 1, nullptr, nullptr, nullptr, nullptr, 2, nullptr, 0, 0, nullptr),
             "eval_ao deriv 2");
  std::printf(failures ? "asan driver: %d failures\n" : "asan driver: ok\n", failures);
  return failures ? 1 : 0;
}
