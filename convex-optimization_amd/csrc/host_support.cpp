// host_support.cpp — the non-inline parts of glx_host.h.
#include "glx_host.h"

#include <cstring>

namespace glx {

void check_workspace(size_t need, const void* ws, size_t wsb, int code, const char* what) {
  if (!ws) throw Error{code, "null workspace"};
  if (wsb < need)
    throw Error{code, what ? std::string("workspace too small (") + what + ")" : std::string("workspace too small")};
  if (reinterpret_cast<uintptr_t>(ws) & 255) throw Error{code, "workspace must be 256-byte aligned"};
}

HostRec::HostRec(size_t n) {
  GLX_HIP(hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(double) * n, hipHostMallocDefault));
}
HostRec::~HostRec() { if (p) (void)hipHostFree(p); }

void check_dtype(int dtype) {
  if (dtype != GLX_F32 && dtype != GLX_F64) throw Error{GLX_E_INVALID, "dtype must be GLX_F32 or GLX_F64"};
}

GemmPlan a_plan(int dtype, int64_t m, int64_t n, int64_t l) {
  glx_problem P;
  glx_opts O;
  std::memset(&P, 0, sizeof P);
  std::memset(&O, 0, sizeof O);
  P.dtype = dtype;
  P.method = GLX_PROXGD;
  P.m = m;
  P.n = n;
  P.l = l;
  O.step_type = GLX_STEP_LINE_SEARCH;
  return session_plan(P, O);
}

std::string plan_field(const GemmPlan& p, int idx) {
  std::string d = describe_plan(p);
  for (int i = 0; i < idx; ++i) {
    const size_t at = d.find("; ");
    d = at == std::string::npos ? std::string() : d.substr(at + 2);
  }
  d = d.substr(0, d.find("; "));
  const size_t eq = d.find('=');
  return eq == std::string::npos ? d : d.substr(eq + 1);
}

bool plan_fuses(const GemmPlan& p, int es) { return atr_prox_ok(p) && (p.atr->fused & dtype_bit(es)) != 0; }

FusePlan fuse_plan(int dtype, int64_t m, int64_t n, int64_t l) {
  FusePlan p;
  p.es = dtype == GLX_F64 ? 8 : 4;
  p.a = a_plan(dtype, m, n, l);
  p.fuse_ok = plan_fuses(p.a, p.es);
  return p;
}

Red glue_red(void* ws, size_t wsb, void* sums_dev, hipStream_t st) {
  Carver c(ws);
  double* part = static_cast<double*>(c.take(sizeof(double) * kMaxRedVals * kMaxBlocks));
  unsigned* ticket = static_cast<unsigned*>(c.take(kTicketBytes));
  check_workspace(c.off, ws, wsb, GLX_E_WORKSPACE, nullptr);
  GLX_HIP(hipMemsetAsync(ticket, 0, kTicketBytes, st));
  return Red{part, ticket, static_cast<double*>(sums_dev)};
}
void check_glue(int dtype, int64_t count, int S) {
  check_dtype(dtype);
  if (count <= 0) throw Error{GLX_E_INVALID, "needs a positive element count"};
  if (S < 1) throw Error{GLX_E_INVALID, "needs S >= 1 slabs"};
}

bool SplitLoop::end_iteration(hipStream_t st) {
  check_launch();
  GLX_HIP(hipMemcpyAsync(host.p, rec, sizeof(double) * nrec, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  ++syncs;
  return step(host.p);
}

void SplitLoop::finish(int64_t k, std::chrono::steady_clock::time_point t0, hipStream_t st, bool count_maxit0_sync) {
  if (k == 0) {
    GLX_HIP(hipMemcpyAsync(host.p, rec, sizeof(double) * split::kRecHead, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    if (count_maxit0_sync) ++syncs;
    f_now = 0.5 * host.p[0] + mu * host.p[1];
  }
  GLX_HIP(hipStreamSynchronize(st));
  res->iters = k;
  res->fval = f_now;
  res->tt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  res->syncs = syncs;
  res->record_waits = 0;
  for (double& sv : res->stats) sv = 0.0;
}

}  // namespace glx
