// Host-side helpers shared by the entry points of libxtddft_amd: error propagation, device
// memory ownership, input upload and the engine runner.  Host only (no device code).
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string>
#include <utility>
#include "../../include/xtddft_amd.h"
#include "xt_internal.h"

namespace xt {

inline int fail(int code, const std::string& msg) { return set_error(code, msg.c_str()); }

// "<what>: " in front of an entry point's messages; the context's ("") carry none
inline std::string err_prefix(const char* what) { return (what && *what) ? std::string(what) + ": " : std::string(); }

#define RET(x) do { int _r = (x); if (_r) return _r; } while (0)
// what: the entry point's message prefix ("" in the context)
#define HIPCHK(what, x) do { hipError_t _e = (x); if (_e != hipSuccess) \
    return xt::fail(XT_ERR_HIP, xt::err_prefix(what) + #x ": " + hipGetErrorString(_e)); } while (0)

// Owner of device memory (n elements of T), grown on demand.  Not copyable; a move leaves
// the source empty.  Freed by release() only: a context keeps its buffers until xt_destroy.
template <class T>
struct DevMem {
  T* p = nullptr;
  size_t n = 0;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  DevMem(DevMem&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  int ensure(size_t count, const char* what = "") {
    if (count <= n) return 0;
    release();
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) {
      p = nullptr;
      return fail(XT_ERR_OOM, err_prefix(what) + "hipMalloc failed for " + std::to_string(count * sizeof(T)) + " bytes");
    }
    n = count;
    return 0;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
  void swap(DevMem& o) { std::swap(p, o.p); std::swap(n, o.n); }
};
// call-scoped form: freed on every return path
template <class T>
struct TmpMem : DevMem<T> {
  ~TmpMem() { this->release(); }
};
using DevBuf = DevMem<double>;
using TmpBuf = TmpMem<double>;

// An input given by a host pointer: copied into b, and p then points at the copy.  Device
// pointers, null pointers and empty inputs pass through untouched.
template <class T>
int upload(TmpMem<T>& b, const T*& p, size_t count, int ptr_kind, hipStream_t st, const char* what) {
  if (ptr_kind != XT_PTR_HOST || !p || count == 0) return 0;
  RET(b.ensure(count, what));
  HIPCHK(what, hipMemcpyAsync(b.p, p, count * sizeof(T), hipMemcpyHostToDevice, st));
  p = b.p;
  return 0;
}

// One engine launch with its split-K workspace: ws grows on demand to min(need, cap) + 8
// bytes (the cap decides dgemm_fit_split and with it the summation order).  hand_max > 0 cuts
// what dgemm() is told it may use.  launch_msg: the message of a rejected launch, after the
// prefix.
inline int run_gemm(const GemmDesc& g, hipStream_t st, DevBuf& ws, size_t cap, size_t hand_max, const char* what,
                    const char* launch_msg) {
  size_t need = dgemm_workspace_bytes(g);
  if (need > cap) need = cap;
  if (need > 0 && ws.n < need / sizeof(double) + 1) {
    HIPCHK(what, hipStreamSynchronize(st));   // an earlier product may still reduce from it
    RET(ws.ensure(need / sizeof(double) + 1, what));
  }
  size_t avail = ws.n * sizeof(double);
  if (hand_max > 0 && avail > hand_max) avail = hand_max;
  const int r = dgemm(g, st, ws.p, avail);
  return r ? fail(r, err_prefix(what) + launch_msg) : 0;
}

// MiB for what grows with the number of states in xt_tdm / xt_tdm_sc (XT_TDM_WS_MIB, default
// 768: a tuning hook, and how the tests reach the chunked path at small sizes)
inline double tdm_budget_mib() {
  double budget = 768.0;
  if (const char* e = getenv("XT_TDM_WS_MIB")) { const double v = atof(e); if (v > 0.0 && v < 768.0) budget = v; }
  return budget;
}

}  // namespace xt
