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
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "glx_host.h"

namespace glx {
namespace {

// the Jacobi sweep, the trace and the stop rule are split_loop.h's (namespace split), shared with
// admm_primal.cpp and alm.cpp; the carver, the pinned record and A's plan are glx_host.h's
using namespace split;
constexpr int kAdmmMaxL = split::kMaxL;

// The launch plans of a solve: A's with its fuse condition (glx_host.h FusePlan); K's is the
// planner's choice for an m x m matrix.
struct AdmmPlan : FusePlan {
  GemmPlan k{};
};
AdmmPlan admm_plan(int dtype, int64_t m, int64_t n, int64_t l, bool with_k = true) {
  check_dtype(dtype);
  if (m <= 0 || n <= 0 || l <= 0) throw Error{GLX_E_INVALID, "m, n, l must be positive"};
  if (l > kAdmmMaxL) throw Error{GLX_E_INVALID, "the dual ADMM solver takes l <= 32"};
  AdmmPlan p;
  static_cast<FusePlan&>(p) = fuse_plan(dtype, m, n, l);
  p.k = with_k ? make_plan(p.es, m, m, l, 0) : p.a;   // (the row step alone plans no K product
  if (!with_k) p.k.ax_S = 1;                            //  and carves one slab for it)
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
  const int ll = (int)(l * l);
  const AdmmPlan pl = admm_plan(P.dtype, m, n, l);
  check_workspace(admm_carve(pl, m, n, l, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_admm_workspace_bytes");
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
  const double mu = P.mu0, rho = O.rho, taurho = O.tau * O.rho;
  SplitLoop loop(rec, l, nl, mu, O.thres, O.converge_len, res);
  int64_t maxit = O.maxit;
  if (O.max_total_iters > 0) maxit = std::min<int64_t>(maxit, O.max_total_iters);

  const auto t0 = std::chrono::steady_clock::now();
  GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
  GLX_HIP(hipMemsetAsync(w.pcnt, 0, sizeof(unsigned) * (n / 64 + 64), st));
  GLX_HIP(hipMemsetAsync(rec, 0, sizeof(double) * loop.nrec, st));
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
  int64_t ax_calls = 1, atr_calls = 0, k_calls = 0;
  int64_t k = 0;
  int cur = 0;
  loop.begin();
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
    const bool stop = loop.end_iteration(st);
    cur = nxt;
    if (stop) break;
  }
  if (cur != 0) GLX_HIP(hipMemcpyAsync(xb[0], xb[1], sizeof(T) * nl, hipMemcpyDeviceToDevice, st));
  loop.finish(k, t0, st, /*count_maxit0_sync=*/true);
  res->ax_calls = ax_calls;
  res->ax_sources = 2 * ax_calls;
  res->atr_calls = atr_calls;
  res->stats[0] = (double)k_calls;       // passes over K
  res->stats[1] = fused ? 1.0 : 0.0;     // the row step ran in the A^T z epilogue
}

}  // namespace
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
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(prob->dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      admm_solve<T>(*prob, static_cast<const T*>(K_device), *opts, ws, wsb, res, st);
    });
  });
}

int glx_admm_trace(double* sparsity_after, int64_t cap, int64_t* n) {
  return guarded([&] {
    const int64_t have = (int64_t)split::trace().size();
    const int64_t k = sparsity_after ? std::min(cap, have) : have;
    for (int64_t i = 0; sparsity_after && i < k; ++i) sparsity_after[i] = split::trace()[(size_t)i];
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
    check_workspace(admm_carve(pl, pl.a.m, n, l, nullptr, nullptr), ws, wsb, GLX_E_WORKSPACE, nullptr);
    AdmmWs w;
    admm_carve(pl, pl.a.m, n, l, ws, &w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    GLX_HIP(hipMemsetAsync(w.pcnt, 0, sizeof(unsigned) * (n / 64 + 64), st));
    Red red{w.part, w.ticket, static_cast<double*>(sums_dev)};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      if (form == 0 && pl.fuse_ok)   // the layout the driver's unfused arm takes at this (m, n, l)
        launch_admm_dual_panel<T>(pl.a, (const T*)x, (const T*)G, 1, nullptr, (T*)u_out, (T*)x_out,
                                  (T*)r_out, rho, tau * rho, mu, red, st);
      else if (form == 0)
        launch_admm_dual<T>((const T*)x, (const T*)G, 1, nullptr, (T*)u_out, (T*)x_out, (T*)r_out, n, l, rho,
                            tau * rho, mu, red, st);
      else
        launch_atr_admm<T>(pl.a, (const T*)A, (const T*)Z, (T*)G, (const T*)x, (T*)u_out, (T*)x_out, (T*)r_out,
                           rho, tau * rho, mu, red, st, pl.a.atr_S > 1 ? (T*)w.gp : nullptr, w.pcnt);
    });
    check_launch();
  });
}

int glx_admm_rhs(int dtype, int64_t ml, const void* Ax, const void* Au, const void* b, double rho, void* v_out,
                 void* stream) {
  return guarded([&] {
    check_glue(dtype, ml, 1);
    if (!Ax || !Au || !b || !v_out) throw Error{GLX_E_INVALID, "null argument"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_admm_v<T>((const T*)Ax, (const T*)Au, (const T*)b, (T*)v_out, ml, rho, st);
    });
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
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_admm_fin<T>((const T*)P, S, (const T*)b, (T*)Ax, (T*)Au, (T*)s, ml, red, st);
    });
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
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_gram<T>((const T*)R, rows, l, (double*)ws, (double*)gram_dev, st);
    });
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
