// alm.cpp — the native driver of the dual ALM solver, gl_Alm_dual(x0, A, b, mu, opts)
// (reference: gl_ALM_dual.py:10-158), beside admm.cpp, with which it shares the outer iteration's
// tail (glx_host.h SplitLoop; split_loop.h, namespace split).
//
// The reference rebuilds, at every outer iteration, the m x m inverse T, F = rho T A, G = I - A^T F,
// Q = F^T F + rho G^T G and J (:33-40), then runs 500 Nesterov steps on grad = Q u + J. Two
// identities ("Dual ALM") leave Q = rho (I + rho A^T A)^-1 =: Qn, built once per solve
// by the caller, and J = rho (A^T K (Ax - b) - x / rho) with K = (I + rho A A^T)^-1. Per outer
// iteration:
//   J      v1 = Ax - b, E = K v1, h = A^T E, J = rho (h - x / rho)            (k_alm_j)
//   inner  inner_iters steps y -> (u, y+) with one pass over Qn each, enqueued back to back: the
//          step in the epilogue of Qn y (k_atr_alm, one launch) or the product and a row kernel
//   z      Au = A u, v = (Ax - rho Au) - b (k_admm_v), z = K v
//   x      g = A^T z, r = u + g, x+ = x - (tau rho) r                         (k_alm_x)
//   record A @ [x+ | u] -> Ax+, ||Ax+ - b||^2, s = Au_prev - Au; the Gram matrices of r and s; one
//          readback; the host takes the two spectral norms and applies the stop rule (:140-148)
// fp64 only.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>

#include "glx_host.h"

namespace glx {
namespace {

using namespace split;

void check_f64(int dtype) {
  if (dtype == GLX_F32)
    throw Error{GLX_E_INVALID,
                "the dual ALM solver is fp64 only: I + rho A^T A has condition number about rho ||A||^2 "
                "(1e5 .. 1e6 at the default rho for m < n), beyond an fp32 inverse applied 500 times per "
                "outer iteration; use GLX_F64"};
  if (dtype != GLX_F64) throw Error{GLX_E_INVALID, "dtype must be GLX_F64"};
}

// The plan of the inner loop: Qn (n x n) in A's place of an A^T R pass with R = y, planned as the
// dual ADMM solver plans A (the tile measured best for a fused epilogue where one fuses).
struct InnerPlan {
  GemmPlan q{};
  bool fuse_ok = false;
};
InnerPlan inner_plan(int dtype, int64_t n, int64_t l) {
  check_f64(dtype);
  if (n <= 0 || l <= 0) throw Error{GLX_E_INVALID, "n, l must be positive"};
  if (l > split::kMaxL) throw Error{GLX_E_INVALID, "the dual ALM solver takes l <= 32"};
  InnerPlan p;
  p.q = a_plan(GLX_F64, n, n, l);
  // The planner splits K up to 64 ways to fill the chip on one long pass; a fused epilogue combines
  // at most 8 slabs (atr_prox_ok). The inner loop is 500 short dependent passes over a matrix that
  // stays in cache, so both of its arms take 8 splits there and the step fuses at every
  // panel-multiple n.
  if (p.q.atr->fam == Fam::Mfma && p.q.atr->wl != 3 && p.q.atr_S > 8) p.q.atr_S = 8;
  p.fuse_ok = plan_fuses(p.q, 8);
  return p;
}
// opts.fused: 0 auto, 1 on (where admitted), 2 off. Auto = on ("Dual ALM").
bool use_fused(const InnerPlan& p, int fused) { return p.fuse_ok && fused != 2; }

struct InnerWs {
  unsigned* pcnt;
  double *y0, *y1, *pq;
};
void inner_carve(const InnerPlan& p, int64_t n, int64_t l, Carver& c, InnerWs* w) {
  w->pcnt = static_cast<unsigned*>(c.take(sizeof(unsigned) * (n / 64 + 64)));
  w->y0 = static_cast<double*>(c.take(8 * n * l));
  w->y1 = static_cast<double*>(c.take(8 * n * l));
  w->pq = static_cast<double*>(c.take(8 * n * l * std::max(1, p.q.atr_S)));   // the slabs of Qn y
}

// The inner loop (:49-63) from u = y = 0: step i has gamma = 2 / (i + 1); the last writes no y+.
// Plain launches on the stream, no host decision in between.
void inner_loop(const InnerPlan& p, bool fused, const double* Qn, const double* J, double* u, const InnerWs& w,
                int64_t n, int64_t l, int iters, double t, double mu, hipStream_t st) {
  double* yb[2] = {w.y0, w.y1};
  const int SQ = p.q.atr_S;
  GLX_HIP(hipMemsetAsync(u, 0, 8 * n * l, st));
  GLX_HIP(hipMemsetAsync(yb[0], 0, 8 * n * l, st));
  int cur = 0;
  for (int i = 1; i <= iters; ++i) {
    const double gamma = 2.0 / (double)(i + 1), gnext = i < iters ? 2.0 / (double)(i + 2) : 0.0;
    double* yn = i < iters ? yb[cur ^ 1] : nullptr;
    if (fused) {
      launch_atr_alm<double>(p.q, Qn, yb[cur], J, u, u, yn, t, mu, gamma, gnext, st, SQ > 1 ? w.pq : nullptr, w.pcnt);
    } else {
      launch_atr<double>(p.q, Qn, yb[cur], w.pq, st);
      if (p.fuse_ok) launch_alm_inner_panel<double>(p.q, w.pq, SQ, yb[cur], J, u, u, yn, t, mu, gamma, gnext, st);
      else launch_alm_inner<double>(w.pq, SQ, yb[cur], J, u, u, yn, n, l, t, mu, gamma, gnext, st);
    }
    cur ^= 1;
  }
}

struct AlmPlan {
  GemmPlan a{}, k{};
  InnerPlan in{};
};
AlmPlan alm_plan(int dtype, int64_t m, int64_t n, int64_t l) {
  check_f64(dtype);
  if (m <= 0 || n <= 0 || l <= 0) throw Error{GLX_E_INVALID, "m, n, l must be positive"};
  if (l > split::kMaxL) throw Error{GLX_E_INVALID, "the dual ALM solver takes l <= 32"};
  AlmPlan p;
  p.a = a_plan(GLX_F64, m, n, l);
  p.k = make_plan(8, m, m, l, 0);
  p.in = inner_plan(dtype, n, l);
  return p;
}

std::string describe_alm(const AlmPlan& p, int fused) {
  std::string s = "K v=" + plan_field(p.k, 0) + "; A u=" + plan_field(p.a, 0) + "; A [x|u]=" + plan_field(p.a, 1) +
                  "; A^T z=" + plan_field(p.a, 3) + "; Qn y=" + plan_field(p.in.q, 3) + "; inner step=";
  s += use_fused(p.in, fused) ? "fused (k_atr_alm, the Qn y epilogue)"
                              : (p.in.fuse_ok ? "row kernel (k_alm_inner_panel, the epilogue's layout)"
                                              : "row kernel (k_alm_inner)");
  return s;
}

struct AlmWs {
  double* part; unsigned* ticket; double* gram_part; double* rec;
  double *u, *J, *r, *gp, *Ax, *Au, *Au1, *s, *v, *z, *pa, *pk;
  InnerWs in;
};
size_t alm_carve(const AlmPlan& p, int64_t m, int64_t n, int64_t l, void* base, AlmWs* out) {
  Carver c(base);
  AlmWs w;
  auto dbl = [&](size_t cnt) { return static_cast<double*>(c.take(sizeof(double) * cnt)); };
  w.part = dbl((size_t)kMaxRedVals * kMaxBlocks);
  w.ticket = static_cast<unsigned*>(c.take(kTicketBytes));
  w.gram_part = dbl((size_t)256 * l * l);
  w.rec = dbl((size_t)(kRecHead + 2 * l * l));
  w.u = dbl(n * l);
  w.J = dbl(n * l);
  w.r = dbl(n * l);
  w.gp = dbl(n * l * std::max(1, p.a.atr_S));   // the K-split slabs of A^T E and A^T z
  w.Ax = dbl(m * l);
  w.Au = dbl(m * l);
  w.Au1 = dbl(m * l);
  w.s = dbl(m * l);
  w.v = dbl(m * l);
  w.z = dbl(m * l);
  w.pa = dbl(m * l * 2 * std::max(1, std::max(ax_split(p.a, 2), ax_split(p.a, 1))));
  w.pk = dbl(m * l * std::max(1, p.k.ax_S));
  inner_carve(p.in, n, l, c, &w.in);
  if (out) *out = w;
  return c.off + 256;
}

void check_opts(const glx_alm_opts* o) {
  if (!o) throw Error{GLX_E_INVALID, "null opts"};
  if (o->maxit < 0 || o->max_total_iters < 0) throw Error{GLX_E_INVALID, "negative iteration limit"};
  if (o->fused < 0 || o->fused > 2) throw Error{GLX_E_INVALID, "fused must be 0 (auto), 1 (on) or 2 (off)"};
  if (!(o->rho > 0.0)) throw Error{GLX_E_INVALID, "rho must be positive"};
  if (o->inner_iters < 1) throw Error{GLX_E_INVALID, "inner_iters must be at least 1"};
}

void alm_solve(const glx_problem& P, const double* K, const double* Qn, const glx_alm_opts& O, void* ws,
               size_t wsb, glx_result* res, hipStream_t st) {
  typedef double T;
  const int64_t m = P.m, n = P.n, l = P.l, nl = n * l, ml = m * l;
  const int ll = (int)(l * l);
  const AlmPlan pl = alm_plan(P.dtype, m, n, l);
  check_workspace(alm_carve(pl, m, n, l, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_alm_workspace_bytes");
  AlmWs w;
  alm_carve(pl, m, n, l, ws, &w);
  const bool fused = use_fused(pl.in, O.fused);
  const int SA2 = ax_split(pl.a, 2), SA1 = ax_split(pl.a, 1), SK = pl.k.ax_S, SG = pl.a.atr_S;
  const T* A = static_cast<const T*>(P.A);
  const T* b = static_cast<const T*>(P.b);
  T* x = static_cast<T*>(P.x);
  double* rec = w.rec;
  const double mu = P.mu0, rho = O.rho, taurho = O.tau * O.rho;
  SplitLoop loop(rec, l, nl, mu, O.thres, O.converge_len, res);
  int64_t maxit = O.maxit;
  if (O.max_total_iters > 0) maxit = std::min<int64_t>(maxit, O.max_total_iters);

  const auto t0 = std::chrono::steady_clock::now();
  GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
  GLX_HIP(hipMemsetAsync(w.in.pcnt, 0, sizeof(unsigned) * (n / 64 + 64), st));
  GLX_HIP(hipMemsetAsync(rec, 0, sizeof(double) * loop.nrec, st));
  GLX_HIP(hipMemsetAsync(w.u, 0, sizeof(T) * nl, st));   // u = 0 (:106)
  auto red = [&](int slot) { return Red{w.part, w.ticket, rec + slot}; };
  auto batched_pass = [&](T* sout) {   // Ax, Au, ||Ax - b||^2 and s = Au_prev - Au
    const T* xs[3] = {x, w.u, nullptr};
    launch_ax<T>(pl.a, 2, A, xs, w.pa, nullptr, 0, st);
    launch_admm_fin<T>(w.pa, SA2, b, w.Ax, w.Au, sout, ml, red(0), st);
  };
  auto k_pass = [&](const T* v, T* out) {   // out = K v
    const T* vs[3] = {v, nullptr, nullptr};
    launch_ax<T>(pl.k, 1, K, vs, SK > 1 ? w.pk : out, nullptr, 0, st);
    if (SK > 1) launch_sum_partials<T>(w.pk, SK, out, ml, st);
  };
  batched_pass(nullptr);
  launch_rownorm_max<T>(x, n, l, red(1), st);   // the objective of x0, returned when maxit = 0
  check_launch();
  int64_t ax_calls = 1, atr_calls = 0, k_calls = 0, inner = 0;
  int64_t k = 0;
  loop.begin();
  while (k < maxit) {
    ++k;
    // J = rho (A^T K (Ax - b) - x / rho); (Ax - 0 Ax) - b is Ax - b
    launch_admm_v<T>(w.Ax, w.Ax, b, w.v, ml, 0.0, st);
    k_pass(w.v, w.z);
    launch_atr<T>(pl.a, A, w.z, w.gp, st);
    launch_alm_j<T>(w.gp, SG, x, w.J, nl, rho, st);
    inner_loop(pl.in, fused, Qn, w.J, w.u, w.in, n, l, O.inner_iters, O.inner_step, mu, st);
    inner += O.inner_iters;
    {   // z = K ((Ax - rho Au) - b) (:120)
      const T* us[3] = {w.u, nullptr, nullptr};
      launch_ax<T>(pl.a, 1, A, us, SA1 > 1 ? w.pa : w.Au1, nullptr, 0, st);
      if (SA1 > 1) launch_sum_partials<T>(w.pa, SA1, w.Au1, ml, st);
      launch_admm_v<T>(w.Ax, w.Au1, b, w.v, ml, rho, st);
      k_pass(w.v, w.z);
    }
    launch_atr<T>(pl.a, A, w.z, w.gp, st);   // g = A^T z, as slabs
    launch_alm_x<T>(x, w.u, w.gp, SG, x, w.r, n, l, taurho, red(1), st);
    batched_pass(w.s);
    ax_calls += 2;
    atr_calls += 2;
    k_calls += 2;
    launch_count_above<T>(x, nl, rec + 2, red(3), st);
    launch_gram<T>(w.r, n, l, w.gram_part, rec + kRecHead, st);
    launch_gram<T>(w.s, m, l, w.gram_part, rec + kRecHead + ll, st);
    if (loop.end_iteration(st)) break;
  }
  loop.finish(k, t0, st, /*count_maxit0_sync=*/false);
  res->ax_calls = ax_calls;
  res->ax_sources = 2 + 3 * k;   // A @ [x0 | 0], then A u and A @ [x+ | u] per iteration
  res->atr_calls = atr_calls;
  res->stats[0] = (double)k_calls;       // passes over K
  res->stats[1] = fused ? 1.0 : 0.0;     // the inner step ran in the Qn y epilogue
  res->stats[2] = (double)inner;         // inner steps run
}

void check_ptr16(std::initializer_list<const void*> ps, const char* what) {
  for (const void* p : ps) {
    if (!p) throw Error{GLX_E_INVALID, std::string(what) + ": null pointer"};
    if (reinterpret_cast<uintptr_t>(p) & 15) throw Error{GLX_E_INVALID, std::string(what) + ": pointers must be 16-byte aligned"};
  }
}

// the workspace of the two kernel-level entries
size_t inner_ws(const InnerPlan& p, int64_t n, int64_t l, void* base, InnerWs* out) {
  Carver c(base);
  InnerWs w;
  inner_carve(p, n, l, c, &w);
  if (out) *out = w;
  return c.off + 256;
}


}  // namespace
}  // namespace glx

using namespace glx;

extern "C" {

int glx_alm_default_opts(glx_alm_opts* o) {
  return guarded([&] {
    if (!o) throw Error{GLX_E_INVALID, "null opts"};
    std::memset(o, 0, sizeof(*o));
    // gl_ALM_dual.py:67-73, :53, :57
    o->maxit = 100;
    o->thres = 1e-3;
    o->tau = (1 + std::sqrt(5.0)) * 0.5;
    o->rho = 1e2;
    o->converge_len = 20;
    o->inner_iters = 500;
    o->inner_step = 1e-2;
  });
}

int glx_alm_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, const glx_alm_opts* opts, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (opts) check_opts(opts);
    *bytes = alm_carve(alm_plan(dtype, m, n, l), m, n, l, nullptr, nullptr);
  });
}

int glx_alm_describe(int dtype, int64_t m, int64_t n, int64_t l, const glx_alm_opts* opts, char* out, size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    if (opts) check_opts(opts);
    std::snprintf(out, cap, "%s", describe_alm(alm_plan(dtype, m, n, l), opts ? opts->fused : 0).c_str());
  });
}

int glx_alm_dual_solve(const glx_problem* prob, const void* K_device, const void* Qn_device,
                       const glx_alm_opts* opts, void* ws, size_t wsb, glx_result* res, void* stream) {
  return guarded([&] {
    if (!prob || !res) throw Error{GLX_E_INVALID, "null problem/result"};
    check_opts(opts);
    if (prob->comm != nullptr) throw Error{GLX_E_INVALID, "the dual ALM solver is single-GPU: comm must be NULL"};
    alm_plan(prob->dtype, prob->m, prob->n, prob->l);   // validates dtype (fp64 only) and shape, before any pointer
    check_ptr16({prob->A, prob->b, prob->x, K_device, Qn_device}, "A, b, x, K, Qn");
    alm_solve(*prob, static_cast<const double*>(K_device), static_cast<const double*>(Qn_device), *opts, ws, wsb,
              res, static_cast<hipStream_t>(stream));
  });
}

int glx_alm_inner_workspace_bytes(int dtype, int64_t n, int64_t l, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    *bytes = inner_ws(inner_plan(dtype, n, l), n, l, nullptr, nullptr);
  });
}

int glx_alm_inner_step(int dtype, int64_t n, int64_t l, const void* Qn, const void* P, int S, const void* y,
                       const void* u, const void* J, double gamma, double gamma_next, double t, double mu,
                       int form, void* u_out, void* y_out, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    const InnerPlan pl = inner_plan(dtype, n, l);
    if (form != 0 && form != 1) throw Error{GLX_E_INVALID, "form must be 0 (row kernel) or 1 (Qn y epilogue)"};
    if (!(gamma > 0.0)) throw Error{GLX_E_INVALID, "gamma must be positive"};
    check_ptr16({y, u, J, u_out}, "y, u, J, u_out");
    if (gamma_next != 0.0) check_ptr16({y_out}, "y_out");
    if (y_out == y) throw Error{GLX_E_INVALID, "y_out must not be y (the product's operand)"};
    if (form == 0) {
      check_ptr16({P}, "P");
      if (S < 1) throw Error{GLX_E_INVALID, "needs S >= 1 slabs"};
    } else {
      check_ptr16({Qn}, "Qn");
      if (!pl.fuse_ok)
        throw Error{GLX_E_INVALID, "form 1: the plan of (n, n, l) takes no fused epilogue (" + describe_plan(pl.q) + ")"};
    }
    check_workspace(inner_ws(pl, n, l, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_alm_inner_workspace_bytes");
    InnerWs w;
    inner_ws(pl, n, l, ws, &w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double *yd = (const double*)y, *ud = (const double*)u, *Jd = (const double*)J;
    double *uo = (double*)u_out, *yo = gamma_next != 0.0 ? (double*)y_out : nullptr;
    if (form == 1) {
      GLX_HIP(hipMemsetAsync(w.pcnt, 0, sizeof(unsigned) * (n / 64 + 64), st));
      launch_atr_alm<double>(pl.q, (const double*)Qn, yd, Jd, ud, uo, yo, t, mu, gamma, gamma_next, st,
                             pl.q.atr_S > 1 ? w.pq : nullptr, w.pcnt);
    } else if (pl.fuse_ok) {
      launch_alm_inner_panel<double>(pl.q, (const double*)P, S, yd, Jd, ud, uo, yo, t, mu, gamma, gamma_next, st);
    } else {
      launch_alm_inner<double>((const double*)P, S, yd, Jd, ud, uo, yo, n, l, t, mu, gamma, gamma_next, st);
    }
    check_launch();
  });
}

int glx_alm_inner_run(int dtype, int64_t n, int64_t l, const void* Qn, const void* J, int iters, double t,
                      double mu, int fused, void* u_out, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    const InnerPlan pl = inner_plan(dtype, n, l);
    if (iters < 1) throw Error{GLX_E_INVALID, "iters must be at least 1"};
    if (fused < 0 || fused > 2) throw Error{GLX_E_INVALID, "fused must be 0 (auto), 1 (on) or 2 (off)"};
    check_ptr16({Qn, J, u_out}, "Qn, J, u_out");
    check_workspace(inner_ws(pl, n, l, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_alm_inner_workspace_bytes");
    InnerWs w;
    inner_ws(pl, n, l, ws, &w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLX_HIP(hipMemsetAsync(w.pcnt, 0, sizeof(unsigned) * (n / 64 + 64), st));
    inner_loop(pl, use_fused(pl, fused), (const double*)Qn, (const double*)J, (double*)u_out, w, n, l, iters, t, mu, st);
    check_launch();
  });
}

int glx_alm_j(int dtype, int64_t nl, int S, const void* h, const void* x, double rho, void* J_out, void* stream) {
  return guarded([&] {
    check_f64(dtype);
    check_glue(dtype, nl, S);
    if (!h || !x || !J_out) throw Error{GLX_E_INVALID, "null argument"};
    if (!(rho > 0.0)) throw Error{GLX_E_INVALID, "rho must be positive"};
    launch_alm_j<double>((const double*)h, S, (const double*)x, (double*)J_out, nl, rho, static_cast<hipStream_t>(stream));
    check_launch();
  });
}

int glx_alm_x(int dtype, int64_t n, int64_t l, int S, const void* x, const void* u, const void* g, double taurho,
              void* x_out, void* r_out, void* sums_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_f64(dtype);
    check_glue(dtype, n, S);
    if (l < 1 || l > split::kMaxL) throw Error{GLX_E_INVALID, "the dual ALM x update takes 1 <= l <= 32"};
    if (!x || !u || !g || !x_out || !r_out || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Red red = glue_red(ws, wsb, sums_dev, st);
    launch_alm_x<double>((const double*)x, (const double*)u, (const double*)g, S, (double*)x_out, (double*)r_out, n, l,
                         taurho, red, st);
    check_launch();
  });
}

}  // extern "C"
