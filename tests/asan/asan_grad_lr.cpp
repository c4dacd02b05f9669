// Host-side sanitizer check of the argument checks of xt_grad_jk2_lr (include/xtddft_amd.h), built by
// tools/asan_grad_lr.sh (every csrc/*.hip with -Xarch_host -fsanitize=address,undefined) and run on a
// machine without a GPU.  A stand-alone program: every rejected call must return XT_ERR_ARG (-1) before the
// first HIP call and leave a message that names the entry; the zero-size calls return 0; xt_grad_jk2
// keeps its own name.  Under ASan / UBSan this covers the message assembly (std::string prefix + text),
// the NaN / inf tests of omega and the workspace arithmetic at the int limits.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include "../../include/xtddft_amd.h"

static int failures = 0;
static const int kErrArg = -1;   // XT_ERR_ARG (csrc/xt_internal.h): what every rejected call returns

static void expect_arg(int rc, const char* entry, const char* word, const char* what) {
  const char* msg = xt_last_error();
  if (rc != kErrArg || msg == nullptr || std::strstr(msg, entry) == nullptr || std::strstr(msg, word) == nullptr) {
    std::printf("FAIL %s: rc %d msg '%s'\n", what, rc, msg ? msg : "(null)");
    ++failures;
  }
}

int main() {
  double d[64] = {0};
  int i[64] = {0};
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  auto lr = [&](int nbra, int nket, int lbra, int lket, int nj, const double* wj, const double* pj, int nk,
                const double* wk, const double* pk, int strip, int natm, double* work, long nwork, double omega) {
    return xt_grad_jk2_lr(nbra, i, d, d, i, nket, i, d, d, i, lbra, lket, nj, wj, pj, pj, nk, wk, pk, pk, 1, strip,
                          natm, work, nwork, d, nullptr, omega);
  };
  const char* E = "xt_grad_jk2_lr";
  const double bad[] = {0.0, -0.0, -0.33, nan, inf, -inf};
  for (double w : bad) {
    expect_arg(lr(1, 1, 3, 2, 2, d, d, 2, d, d, 1, 1, d, 6, w), E, "omega", "omega not finite and > 0");
    expect_arg(lr(0, 1, 3, 2, 2, d, d, 2, d, d, 1, 1, d, 6, w), E, "omega", "omega refused on a zero-size call");
  }
  expect_arg(lr(-1, 1, 3, 2, 2, d, d, 2, d, d, 1, 1, d, 6, 0.33), E, "negative size", "nbra < 0");
  expect_arg(lr(1, 1, 3, 2, 2, d, d, 2, d, d, 1, 1, d, -1, 0.33), E, "negative size", "nwork < 0");
  expect_arg(lr(1, 1, 3, 2, 2, d, d, 2, d, d, 0, 1, d, 6, 0.33), E, "strip", "strip 0");
  expect_arg(lr(1, 1, 9, 0, 2, d, d, 2, d, d, 1, 1, d, 6, 0.33), E, "order", "bra order 9");
  expect_arg(lr(1, 1, 8, 7, 2, d, d, 2, d, d, 1, 1, d, 6, 0.33), E, "order", "total order 15");
  expect_arg(lr(1, 1, 3, 2, 9, d, d, 2, d, d, 1, 1, d, 6, 0.33), E, "nj", "nj 9");
  expect_arg(lr(1, 1, 3, 2, 2, d, d, -1, d, d, 1, 1, d, 6, 0.33), E, "nk", "nk -1");
  expect_arg(lr(1, 1, 3, 2, 0, nullptr, nullptr, 0, nullptr, nullptr, 1, 1, d, 6, 0.33), E, "both zero", "no pair");
  expect_arg(lr(1, 1, 3, 2, 2, nullptr, d, 2, d, d, 1, 1, d, 6, 0.33), E, "wj", "null wj");
  expect_arg(lr(1, 1, 3, 2, 0, nullptr, nullptr, 2, nullptr, d, 1, 1, d, 6, 0.33), E, "wk", "null wk");
  expect_arg(lr(1, 1, 3, 2, 0, nullptr, nullptr, 2, d, nullptr, 1, 1, d, 6, 0.33), E, "pk or qk", "null pk");
  expect_arg(lr(1, 1, 3, 2, 0, nullptr, nullptr, 2, d, d, 1, 1, nullptr, 6, 0.33), E, "null", "null work");
  expect_arg(lr(1, 1, 3, 2, 0, nullptr, nullptr, 2, d, d, 1, 1, d, 5, 0.33), E, "workspace", "nwork one short");
  expect_arg(lr(1, 5, 3, 2, 0, nullptr, nullptr, 2, d, d, 2, 1, d, 11, 0.33), E, "workspace", "three strips + 1");
  expect_arg(lr(1, 5, 3, 2, 0, nullptr, nullptr, 2, d, d, std::numeric_limits<int>::max(), 1, d, 5, 0.33), E,
             "workspace", "strip at INT_MAX");
  if (lr(0, 1, 3, 2, 2, d, d, 2, d, d, 1, 1, d, 6, 0.33) != 0 || lr(1, 0, 3, 2, 2, d, d, 2, d, d, 1, 1, d, 6, 0.33) != 0 ||
      lr(1, 1, 3, 2, 0, nullptr, nullptr, 2, d, d, 1, 0, d, 6, 0.2) != 0) {
    std::printf("FAIL zero-size calls return 0\n");
    ++failures;
  }
  // the full-range entry shares the checks and keeps its own name
  expect_arg(xt_grad_jk2(1, i, d, d, i, 1, i, d, d, i, 3, 2, 2, d, d, d, 2, d, d, d, 1, 1, 1, d, 5, d, nullptr),
             "xt_grad_jk2:", "workspace", "xt_grad_jk2 names itself");
  std::printf(failures ? "asan grad_lr: %d failures\n" : "asan grad_lr: ok\n", failures);
  return failures ? 1 : 0;
}
