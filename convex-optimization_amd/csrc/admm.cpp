// admm.cpp — the native driver of the dual ADMM solver, gl_Admm_dual(x0, A, b, mu, opts)
// (reference: gl_ADMM_dual.py:10-103), beside solver.cpp's Session<T> and independent of it.
//
// The reference solves with the Cholesky factor of I + rho A A^T at every iteration (:57, :63).
// Two triangular solves with l <= 32 right-hand sides are a chain of dependent steps on a GPU, so
// the caller hands in the explicit inverse K = (I + rho A A^T)^-1 (built once per solve, in fp64,
// by the Python layer) and z = K v is one more dense product through launch_ax, with K in A's
// place. Per iteration: one pass over K, two over A (g = A^T z with the row step in its epilogue
// where the plan fuses; A @ [x+ | u+] batched), a handful of small kernels, and one readback of
// a small record: the objective's two sums, the count for the logged sparsity and the two l x l
// Gram matrices r^T r, s^T s, whose largest eigenvalues (a cyclic Jacobi sweep on the host) give
// the spectral norms of the stop rule (:85-93).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "glx.h"
#include "glx_internal.h"

namespace glx {
namespace {

#define GLX_HIP(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) throw Error{GLX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)}; \
  } while (0)

inline void check_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw Error{GLX_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e)};
}

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

// the carver, the pinned record, the Jacobi sweep and the trace are shared with admm_primal.cpp
// (glx_internal.h, namespace admm; defined at the end of this file)
using namespace admm;
constexpr int kAdmmMaxL = admm::kMaxL;

// The launch plans of a solve: A's is the session plan of a one-GPU line-search ProxGD at this
// shape, i.e. the A^T R tile and split measured best for a fused epilogue where one fuses (both
// forms of the row step run on it, so they see the same bits of g); K's is the planner's choice
// for an m x m matrix. fuse_ok: the plan takes a fused epilogue and its tile is built for it.
struct AdmmPlan {
  int es = 8;
  GemmPlan a{}, k{};
  bool fuse_ok = false;
};
AdmmPlan admm_plan(int dtype, int64_t m, int64_t n, int64_t l, bool with_k = true) {
  if (dtype != GLX_F32 && dtype != GLX_F64) throw Error{GLX_E_INVALID, "dtype must be GLX_F32 or GLX_F64"};
  if (m <= 0 || n <= 0 || l <= 0) throw Error{GLX_E_INVALID, "m, n, l must be positive"};
  if (l > kAdmmMaxL) throw Error{GLX_E_INVALID, "the dual ADMM solver takes l <= 32"};
  AdmmPlan p;
  p.es = dtype == GLX_F64 ? 8 : 4;
  p.a = admm::a_plan(dtype, m, n, l);
  p.k = with_k ? make_plan(p.es, m, m, l, 0) : p.a;   // (the row step alone plans no K product
  if (!with_k) p.k.ax_S = 1;                            //  and carves one slab for it)
  p.fuse_ok = atr_prox_ok(p.a) && (p.a.atr->fused & dtype_bit(p.es)) != 0;
  return p;
}
// opts.fused: 0 auto, 1 on (where admitted), 2 off. Auto = on: the A/B at (8192, 16384, 32) fp64
// measured the fused epilogue not slower than the row kernel ("Dual ADMM").
bool use_fused(const AdmmPlan& p, int fused) { return p.fuse_ok && fused != 2; }

std::string describe_admm(const AdmmPlan& p, int fused) {
  std::string s = "K v=" + plan_field(p.k, 0) + "; A [x|u]=" + plan_field(p.a, 1) + "; A^T z=" +
                  plan_field(p.a, 3) + "; projection=";
  s += use_fused(p, fused) ? "fused (k_atr_admm, the A^T z epilogue)"
                           : (p.fuse_ok ? "row kernel (k_admm_dual_panel, the epilogue's layout)" : "row kernel (k_admm_dual)");
  return s;
}

struct AdmmWs {
  double* part; unsigned* ticket; unsigned* pcnt; void* g; void* gp; double* gram_part; double* rec;
  void *x1, *u0, *u1, *r, *Ax, *Au, *s, *v, *z, *pa, *pk;
};
size_t admm_carve(const AdmmPlan& p, int64_t m, int64_t n, int64_t l, void* base, AdmmWs* out) {
  Carver c(base);
  const size_t es = (size_t)p.es;
  AdmmWs w;
  w.part = static_cast<double*>(c.take(sizeof(double) * kMaxRedVals * kMaxBlocks));
  w.ticket = static_cast<unsigned*>(c.take(kTicketBytes));
  w.pcnt = static_cast<unsigned*>(c.take(sizeof(unsigned) * (n / 64 + 64)));
  w.g = c.take(es * n * l);
  w.gp = c.take(es * n * l * std::max(1, p.a.atr_S));   // the K-split slabs of A^T z
  w.gram_part = static_cast<double*>(c.take(sizeof(double) * 256 * l * l));
  w.rec = static_cast<double*>(c.take(sizeof(double) * (kRecHead + 2 * l * l)));
  w.x1 = c.take(es * n * l);
  w.u0 = c.take(es * n * l);
  w.u1 = c.take(es * n * l);
  w.r = c.take(es * n * l);
  w.Ax = c.take(es * m * l);
  w.Au = c.take(es * m * l);
  w.s = c.take(es * m * l);
  w.v = c.take(es * m * l);
  w.z = c.take(es * m * l);
  w.pa = c.take(es * m * l * 2 * std::max(1, ax_split(p.a, 2)));
  w.pk = c.take(es * m * l * std::max(1, p.k.ax_S));
  if (out) *out = w;
  return c.off + 256;
}

void check_opts(const glx_admm_opts* o) {
  if (!o) throw Error{GLX_E_INVALID, "null opts"};
  if (o->maxit < 0 || o->max_total_iters < 0) throw Error{GLX_E_INVALID, "negative iteration limit"};
  if (o->fused < 0 || o->fused > 2) throw Error{GLX_E_INVALID, "fused must be 0 (auto), 1 (on) or 2 (off)"};
  if (!(o->rho > 0.0)) throw Error{GLX_E_INVALID, "rho must be positive"};
}

template <typename T>
void admm_solve(const glx_problem& P, const T* K, const glx_admm_opts& O, void* ws, size_t wsb,
                glx_result* res, hipStream_t st) {
  const int64_t m = P.m, n = P.n, l = P.l, nl = n * l, ml = m * l;
  const int ll = (int)(l * l), nrec = kRecHead + 2 * ll;
  const AdmmPlan pl = admm_plan(P.dtype, m, n, l);
  if (wsb < admm_carve(pl, m, n, l, nullptr, nullptr)) throw Error{GLX_E_INVALID, "workspace too small (glx_admm_workspace_bytes)"};
  if (reinterpret_cast<uintptr_t>(ws) & 255) throw Error{GLX_E_INVALID, "workspace must be 256-byte aligned"};
  AdmmWs w;
  admm_carve(pl, m, n, l, ws, &w);
  const bool fused = use_fused(pl, O.fused);
  const int SA = ax_split(pl.a, 2), SK = pl.k.ax_S, SG = pl.a.atr_S;
  const T* A = static_cast<const T*>(P.A);
  const T* b = static_cast<const T*>(P.b);
  T* xb[2] = {static_cast<T*>(P.x), static_cast<T*>(w.x1)};
  T* ub[2] = {static_cast<T*>(w.u0), static_cast<T*>(w.u1)};
  T *r = static_cast<T*>(w.r), *Ax = static_cast<T*>(w.Ax), *Au = static_cast<T*>(w.Au);
  T *s = static_cast<T*>(w.s), *v = static_cast<T*>(w.v), *z = static_cast<T*>(w.z);
  T *pa = static_cast<T*>(w.pa), *pk = static_cast<T*>(w.pk), *g = static_cast<T*>(w.g), *gp = static_cast<T*>(w.gp);
  double* rec = w.rec;
  HostRec host((size_t)nrec);
  int64_t maxit = O.maxit;
  if (O.max_total_iters > 0) maxit = std::min<int64_t>(maxit, O.max_total_iters);
  const double mu = P.mu0, rho = O.rho, taurho = O.tau * O.rho;

  const auto t0 = std::chrono::steady_clock::now();
  GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
  GLX_HIP(hipMemsetAsync(w.pcnt, 0, sizeof(unsigned) * (n / 64 + 64), st));
  GLX_HIP(hipMemsetAsync(rec, 0, sizeof(double) * nrec, st));
  GLX_HIP(hipMemsetAsync(ub[0], 0, sizeof(T) * nl, st));   // u = 0 (:50)
  auto red = [&](int slot) { return Red{w.part, w.ticket, rec + slot}; };
  auto batched_pass = [&](const T* x, const T* u, T* sout) {
    const T* xs[3] = {x, u, nullptr};
    launch_ax<T>(pl.a, 2, A, xs, pa, nullptr, 0, st);
    launch_admm_fin<T>(pa, SA, b, Ax, Au, sout, ml, red(0), st);
  };
  batched_pass(xb[0], ub[0], nullptr);
  launch_rownorm_max<T>(xb[0], n, l, red(1), st);   // the objective of x0, returned when maxit = 0
  check_launch();
  int64_t ax_calls = 1, atr_calls = 0, k_calls = 0, syncs = 0;
  int64_t k = 0, length = 0;
  int cur = 0;
  double f_best = std::numeric_limits<double>::infinity(), f_now = 0.0;
  admm::trace().clear();
  res->n_fhist = 0;
  while (k < maxit) {
    ++k;
    const int nxt = cur ^ 1;
    launch_admm_v<T>(Ax, Au, b, v, ml, rho, st);
    {   // z = K v
      const T* vs[3] = {v, nullptr, nullptr};
      launch_ax<T>(pl.k, 1, K, vs, SK > 1 ? pk : z, nullptr, 0, st);
      if (SK > 1) launch_sum_partials<T>(pk, SK, z, ml, st);
      ++k_calls;
    }
    if (fused) {
      launch_atr_admm<T>(pl.a, A, z, g, xb[cur], ub[nxt], xb[nxt], r, rho, taurho, mu, red(1), st,
                         SG > 1 ? gp : nullptr, w.pcnt);
    } else {
      // the row kernel on the slabs: where the plan would fuse, on the epilogue's panel layout,
      // so that fused = 1 and fused = 2 give the same bits (the sums' order included)
      launch_atr<T>(pl.a, A, z, gp, st);
      if (pl.fuse_ok)
        launch_admm_dual_panel<T>(pl.a, xb[cur], gp, SG, nullptr, ub[nxt], xb[nxt], r, rho, taurho, mu, red(1), st);
      else
        launch_admm_dual<T>(xb[cur], gp, SG, nullptr, ub[nxt], xb[nxt], r, n, l, rho, taurho, mu, red(1), st);
    }
    ++atr_calls;
    batched_pass(xb[nxt], ub[nxt], s);
    ++ax_calls;
    launch_count_above<T>(xb[nxt], nl, rec + 2, red(3), st);
    launch_gram<T>(r, n, l, w.gram_part, rec + kRecHead, st);
    launch_gram<T>(s, m, l, w.gram_part, rec + kRecHead + ll, st);
    check_launch();
    GLX_HIP(hipMemcpyAsync(host.p, rec, sizeof(double) * nrec, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    ++syncs;
    cur = nxt;
    const double* h = host.p;
    f_now = 0.5 * h[0] + mu * h[1];
    f_best = f_now < f_best ? f_now : f_best;   // min(f_best, f_now): a NaN f_now is not taken
    if (res->f_hist && res->n_fhist < res->f_cap) {
      res->f_hist[res->n_fhist] = f_now;
      if (res->f_hist_best) res->f_hist_best[res->n_fhist] = f_best;
      ++res->n_fhist;
    }
    admm::trace().push_back(h[3] / (double)nl);
    const double rn = spectral_norm(h + kRecHead, (int)l), sn = spectral_norm(h + kRecHead + ll, (int)l);
    if (rn < O.thres && sn < O.thres) ++length;
    else length = 0;
    if (length >= O.converge_len) break;
  }
  if (k == 0) {
    GLX_HIP(hipMemcpyAsync(host.p, rec, sizeof(double) * kRecHead, hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    ++syncs;
    f_now = 0.5 * host.p[0] + mu * host.p[1];
  }
  if (cur != 0) GLX_HIP(hipMemcpyAsync(xb[0], xb[1], sizeof(T) * nl, hipMemcpyDeviceToDevice, st));
  GLX_HIP(hipStreamSynchronize(st));
  res->iters = k;
  res->fval = f_now;
  res->tt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  res->ax_calls = ax_calls;
  res->ax_sources = 2 * ax_calls;
  res->atr_calls = atr_calls;
  res->syncs = syncs;
  res->record_waits = 0;
  for (double& sv : res->stats) sv = 0.0;
  res->stats[0] = (double)k_calls;       // passes over K
  res->stats[1] = fused ? 1.0 : 0.0;     // the row step ran in the A^T z epilogue
}


// the workspace of the glue-kernel entries: the reduction's partials and its arrival tickets
Red glue_red(void* ws, size_t wsb, void* sums_dev, hipStream_t st) {
  Carver c(ws);
  double* part = static_cast<double*>(c.take(sizeof(double) * kMaxRedVals * kMaxBlocks));
  unsigned* ticket = static_cast<unsigned*>(c.take(kTicketBytes));
  if (!ws || wsb < c.off) throw Error{GLX_E_WORKSPACE, "workspace too small"};
  if (reinterpret_cast<uintptr_t>(ws) & 255) throw Error{GLX_E_WORKSPACE, "workspace must be 256-byte aligned"};
  GLX_HIP(hipMemsetAsync(ticket, 0, kTicketBytes, st));
  return Red{part, ticket, static_cast<double*>(sums_dev)};
}
void check_glue(int dtype, int64_t count, int S) {
  if (dtype != GLX_F32 && dtype != GLX_F64) throw Error{GLX_E_INVALID, "dtype must be GLX_F32 or GLX_F64"};
  if (count <= 0) throw Error{GLX_E_INVALID, "needs a positive element count"};
  if (S < 1) throw Error{GLX_E_INVALID, "needs S >= 1 slabs"};
}

}  // namespace

// ---- shared with admm_primal.cpp (glx_internal.h, namespace admm) ----
namespace admm {

// Largest eigenvalue of the symmetric l x l matrix G (row-major) by cyclic Jacobi sweeps
// (Golub & Van Loan, Alg. 8.5.3); NaN where G holds one. The Gram matrices of the stop rule are
// at most 32 x 32, so a sweep is a few thousand flops on the host.
double sym_lambda_max(const double* G, int l) {
  double a[kMaxL][kMaxL];
  double tr = 0.0;
  for (int i = 0; i < l; ++i)
    for (int j = 0; j < l; ++j) {
      const double v = G[i * l + j];
      if (v != v) return std::numeric_limits<double>::quiet_NaN();
      a[i][j] = v;
      if (i == j) tr += std::fabs(v);
    }
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < l; ++p)
      for (int q = p + 1; q < l; ++q) off += a[p][q] * a[p][q];
    if (!(std::sqrt(off) > 1e-18 * tr)) break;
    for (int p = 0; p < l; ++p)
      for (int q = p + 1; q < l; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
        for (int k = 0; k < l; ++k) {
          if (k == p || k == q) continue;
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = a[p][k] = cs * akp - sn * akq;
          a[k][q] = a[q][k] = sn * akp + cs * akq;
        }
        a[p][p] -= t * apq;
        a[q][q] += t * apq;
        a[p][q] = a[q][p] = 0.0;
      }
  }
  double mx = a[0][0];
  for (int i = 1; i < l; ++i) mx = a[i][i] > mx ? a[i][i] : mx;
  return mx;
}
// the spectral norm of R from R^T R (a tiny negative eigenvalue of a rounded Gram matrix is 0)
double spectral_norm(const double* gram, int l) {
  const double lm = sym_lambda_max(gram, l);
  return lm != lm ? lm : std::sqrt(lm > 0.0 ? lm : 0.0);
}

std::vector<double>& trace() {
  thread_local std::vector<double> sparsity;
  return sparsity;
}

HostRec::HostRec(size_t n) { GLX_HIP(hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(double) * n, hipHostMallocDefault)); }
HostRec::~HostRec() { if (p) (void)hipHostFree(p); }

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

}  // namespace admm

}  // namespace glx

using namespace glx;

extern "C" {

int glx_admm_default_opts(glx_admm_opts* o) {
  return guarded([&] {
    if (!o) throw Error{GLX_E_INVALID, "null opts"};
    std::memset(o, 0, sizeof(*o));
    // gl_ADMM_dual.py:11-17
    o->maxit = 100;
    o->thres = 1e-3;
    o->tau = (1 + std::sqrt(5.0)) * 0.5;
    o->rho = 1e2;
    o->converge_len = 20;
  });
}

int glx_admm_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, const glx_admm_opts* opts,
                             size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (opts) check_opts(opts);
    *bytes = admm_carve(admm_plan(dtype, m, n, l), m, n, l, nullptr, nullptr);
  });
}

int glx_admm_describe(int dtype, int64_t m, int64_t n, int64_t l, const glx_admm_opts* opts, char* out,
                      size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    if (opts) check_opts(opts);
    std::snprintf(out, cap, "%s", describe_admm(admm_plan(dtype, m, n, l), opts ? opts->fused : 0).c_str());
  });
}

int glx_admm_dual_solve(const glx_problem* prob, const void* K_device, const glx_admm_opts* opts,
                        void* ws, size_t wsb, glx_result* res, void* stream) {
  return guarded([&] {
    if (!prob || !res) throw Error{GLX_E_INVALID, "null problem/result"};
    check_opts(opts);
    if (prob->comm != nullptr) throw Error{GLX_E_INVALID, "the dual ADMM solver is single-GPU: comm must be NULL"};
    if (!prob->A || !prob->b || !prob->x) throw Error{GLX_E_INVALID, "A, b and x must be device pointers"};
    if (!K_device) throw Error{GLX_E_INVALID, "K (the inverse of I + rho A A^T) must be a device pointer"};
    if ((reinterpret_cast<uintptr_t>(prob->A) | reinterpret_cast<uintptr_t>(prob->b) |
         reinterpret_cast<uintptr_t>(prob->x) | reinterpret_cast<uintptr_t>(K_device)) & 15)
      throw Error{GLX_E_INVALID, "A, b, x, K must be 16-byte aligned"};
    admm_plan(prob->dtype, prob->m, prob->n, prob->l);   // validates dtype and shape
    if (!ws) throw Error{GLX_E_INVALID, "null workspace"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (prob->dtype == GLX_F64) admm_solve<double>(*prob, static_cast<const double*>(K_device), *opts, ws, wsb, res, st);
    else admm_solve<float>(*prob, static_cast<const float*>(K_device), *opts, ws, wsb, res, st);
  });
}

int glx_admm_trace(double* sparsity_after, int64_t cap, int64_t* n) {
  return guarded([&] {
    const int64_t have = (int64_t)admm::trace().size();
    const int64_t k = sparsity_after ? std::min(cap, have) : have;
    for (int64_t i = 0; sparsity_after && i < k; ++i) sparsity_after[i] = admm::trace()[(size_t)i];
    if (n) *n = k;
  });
}

int glx_admm_dual_step(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* Z, void* G,
                       const void* x, double rho, double tau, double mu, int form, void* u_out,
                       void* x_out, void* r_out, void* sums_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    if (form != 0 && form != 1) throw Error{GLX_E_INVALID, "form must be 0 (row kernel) or 1 (A^T z epilogue)"};
    const AdmmPlan pl = admm_plan(dtype, m, n, l, false);
    if (!G || !x || !u_out || !x_out || !r_out || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    if (form == 1) {
      if (!A || !Z) throw Error{GLX_E_INVALID, "form 1 needs A and Z"};
      if (!pl.fuse_ok)
        throw Error{GLX_E_INVALID, "form 1: this shape's A^T R plan takes no fused epilogue (" + describe_plan(pl.a) + ")"};
    }
    if (!ws || wsb < admm_carve(pl, pl.a.m, n, l, nullptr, nullptr)) throw Error{GLX_E_WORKSPACE, "workspace too small"};
    if (reinterpret_cast<uintptr_t>(ws) & 255) throw Error{GLX_E_WORKSPACE, "workspace must be 256-byte aligned"};
    AdmmWs w;
    admm_carve(pl, pl.a.m, n, l, ws, &w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    GLX_HIP(hipMemsetAsync(w.pcnt, 0, sizeof(unsigned) * (n / 64 + 64), st));
    Red red{w.part, w.ticket, static_cast<double*>(sums_dev)};
    auto go = [&](auto* tag) {
      typedef std::remove_pointer_t<decltype(tag)> T;
      if (form == 0 && pl.fuse_ok)   // the layout the driver's unfused arm takes at this (m, n, l)
        launch_admm_dual_panel<T>(pl.a, (const T*)x, (const T*)G, 1, nullptr, (T*)u_out, (T*)x_out,
                                  (T*)r_out, rho, tau * rho, mu, red, st);
      else if (form == 0)
        launch_admm_dual<T>((const T*)x, (const T*)G, 1, nullptr, (T*)u_out, (T*)x_out, (T*)r_out, n, l, rho,
                            tau * rho, mu, red, st);
      else
        launch_atr_admm<T>(pl.a, (const T*)A, (const T*)Z, (T*)G, (const T*)x, (T*)u_out, (T*)x_out, (T*)r_out,
                           rho, tau * rho, mu, red, st, pl.a.atr_S > 1 ? (T*)w.gp : nullptr, w.pcnt);
    };
    if (dtype == GLX_F64) go(static_cast<double*>(nullptr));
    else go(static_cast<float*>(nullptr));
    check_launch();
  });
}

int glx_admm_rhs(int dtype, int64_t ml, const void* Ax, const void* Au, const void* b, double rho, void* v_out,
                 void* stream) {
  return guarded([&] {
    check_glue(dtype, ml, 1);
    if (!Ax || !Au || !b || !v_out) throw Error{GLX_E_INVALID, "null argument"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == GLX_F64) launch_admm_v<double>((const double*)Ax, (const double*)Au, (const double*)b, (double*)v_out, ml, rho, st);
    else launch_admm_v<float>((const float*)Ax, (const float*)Au, (const float*)b, (float*)v_out, ml, rho, st);
    check_launch();
  });
}

int glx_admm_fin(int dtype, int64_t ml, int S, const void* P, const void* b, void* Ax, void* Au, void* s,
                 void* sums_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_glue(dtype, ml, S);
    if (!P || !b || !Ax || !Au || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Red red = glue_red(ws, wsb, sums_dev, st);
    if (dtype == GLX_F64) launch_admm_fin<double>((const double*)P, S, (const double*)b, (double*)Ax, (double*)Au, (double*)s, ml, red, st);
    else launch_admm_fin<float>((const float*)P, S, (const float*)b, (float*)Ax, (float*)Au, (float*)s, ml, red, st);
    check_launch();
  });
}

int glx_gram(int dtype, int64_t rows, int64_t l, const void* R, void* gram_dev, void* ws, size_t wsb,
             void* stream) {
  return guarded([&] {
    if (dtype != GLX_F32 && dtype != GLX_F64) throw Error{GLX_E_INVALID, "bad dtype"};
    if (rows <= 0 || l <= 0 || l > kAdmmMaxL) throw Error{GLX_E_INVALID, "needs rows > 0 and 1 <= l <= 32"};
    if (!R || !gram_dev) throw Error{GLX_E_INVALID, "null argument"};
    if (!ws || wsb < sizeof(double) * 256 * l * l) throw Error{GLX_E_WORKSPACE, "workspace too small"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == GLX_F64) launch_gram<double>((const double*)R, rows, l, (double*)ws, (double*)gram_dev, st);
    else launch_gram<float>((const float*)R, rows, l, (double*)ws, (double*)gram_dev, st);
    check_launch();
  });
}

int glx_sym_lambda_max(const double* G, int l, double* out) {
  return guarded([&] {
    if (!G || !out || l < 1 || l > kAdmmMaxL) throw Error{GLX_E_INVALID, "needs G, out and 1 <= l <= 32"};
    *out = sym_lambda_max(G, l);
  });
}

}  // extern "C"
