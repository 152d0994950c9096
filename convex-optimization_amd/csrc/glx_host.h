// glx_host.h — what the native drivers (solver.cpp, admm.cpp, admm_primal.cpp, alm.cpp,
// certificate.cpp, screen.cpp, group.cpp) share on the host: the HIP error check, the C ABI's
// exception boundary, the workspace carver and its check, the dtype dispatch, A's plan with its
// fuse condition, and the split solvers' readback loop. Host only: no .hip file includes it.
// The non-inline parts are in host_support.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <exception>
#include <string>

#include "glx.h"
#include "glx_internal.h"
#include "split_loop.h"

namespace glx {

#define GLX_HIP(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) throw Error{GLX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)}; \
  } while (0)

inline void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw Error{GLX_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e)};
}

// the body of a C entry: an exception becomes its return code and glx_last_error()
template <typename F>
int guarded(F&& f) {
  try {
    f();
    return GLX_OK;
  } catch (const Error& e) {
    g_last_error = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return GLX_E_STATE;
  } catch (...) {
    g_last_error = "unknown error";
    return GLX_E_STATE;
  }
}

struct Carver {   // 256-byte aligned pieces of a workspace (base == NULL: sizes only)
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base(static_cast<char*>(b)) {}
  void* take(size_t bytes) {
    off = (off + 255) & ~size_t(255);
    void* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  }
};
// A caller's workspace: not null, at least `need` bytes, 256-byte aligned. `code` is the family's:
// GLX_E_INVALID in the solvers, the certificate, the certified solve, the group entries and their
// one-launch steps; GLX_E_WORKSPACE in the session, the single-kernel entries of solver.cpp and
// the ADMM / ALM glue and row-step entries (include/glx.h documents both). `what` (may be NULL)
// names the entry that reports the size.
void check_workspace(size_t need, const void* ws, size_t wsb, int code, const char* what);

struct HostRec {   // n pinned doubles for the per-iteration readback
  double* p = nullptr;
  explicit HostRec(size_t n);
  ~HostRec();
  HostRec(const HostRec&) = delete;
  HostRec& operator=(const HostRec&) = delete;
};

void check_dtype(int dtype);   // GLX_E_INVALID unless GLX_F32 or GLX_F64
// f(DType<double>{}) or f(DType<float>{}) by an (already checked) dtype:
//   by_dtype(dtype, [&](auto tag) { using T = typename decltype(tag)::type; launch_x<T>(..); });
template <typename T>
struct DType {
  using type = T;
};
template <typename F>
decltype(auto) by_dtype(int dtype, F&& f) {
  if (dtype == GLX_F64) return f(DType<double>{});
  return f(DType<float>{});
}

// A's plan outside a session: the session plan of a one-GPU line-search ProxGD at this shape, i.e.
// the A^T R tile and split measured best for a fused epilogue where one fuses
GemmPlan a_plan(int dtype, int64_t m, int64_t n, int64_t l);
// field `idx` of describe_plan's "ax1=..; ax2=..; ax3=..; atr=.." line, without its label
std::string plan_field(const GemmPlan& p, int idx);
// the plan takes a fused A^T R epilogue and its tile is built for one at this element size
bool plan_fuses(const GemmPlan& p, int es);
// a_plan with its element size and fuse condition: what the dual ADMM solver, the certificate and
// the certified solve launch A by (both forms of a row step run on it, so they see the same bits)
struct FusePlan {
  int es = 8;
  GemmPlan a{};
  bool fuse_ok = false;
};
FusePlan fuse_plan(int dtype, int64_t m, int64_t n, int64_t l);

// the workspace of a glue-kernel entry: the reduction's partials and its arrival tickets (zeroed
// on st), summing into sums_dev; and the checks of such an entry's dtype, count and slabs
Red glue_red(void* ws, size_t wsb, void* sums_dev, hipStream_t st);
void check_glue(int dtype, int64_t count, int S);

// The tail of an outer iteration of the three split solvers (admm.cpp, admm_primal.cpp, alm.cpp):
// the record [||Ax - b||^2, sum_i ||x_i||, max |x|, count] + two l x l Gram matrices comes back
// from `rec` once per iteration and split::SplitTail (split_loop.h) takes the objective, the
// histories, the sparsity trace, the two spectral norms and the stop rule from it.
struct SplitLoop : split::SplitTail {
  HostRec host;
  double* rec;   // device, nrec doubles
  int nrec;
  int64_t syncs = 0;
  SplitLoop(double* rec_dev, int64_t l, int64_t nl, double mu, double thres, int64_t converge_len, glx_result* res)
      : split::SplitTail{mu, thres, converge_len, nl, l, res},
        host((size_t)(split::kRecHead + 2 * l * l)),
        rec(rec_dev),
        nrec((int)(split::kRecHead + 2 * l * l)) {}
  // after an iteration's launches: the launch check, the record's copy, the wait; true = stop
  bool end_iteration(hipStream_t st);
  // after the loop (and anything the solver queued behind it): with k = 0 the objective of x0 from
  // the record's head, the last wait, and the result's fields every solver fills alike. The
  // solver's own counters and stats[0..2] follow. count_maxit0_sync: whether the k = 0 readback
  // counts in res->syncs (the dual ADMM solver's does, the other two's do not)
  void finish(int64_t k, std::chrono::steady_clock::time_point t0, hipStream_t st, bool count_maxit0_sync);
};

}  // namespace glx
