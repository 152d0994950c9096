// admm_primal.cpp — the native driver of the primal ADMM solver, gl_Admm_primal(x0, A, b, mu, opts)
// (reference: gl_ADMM_primal.py:10-117), beside admm.cpp, with which it shares the outer iteration's
// tail (glx_host.h SplitLoop; split_loop.h, namespace split).
//
// The reference solves with the Cholesky factor of rho I + A^T A (n x n) at every iteration (:62,
// :78). Here y+ = (rho I + A^T A)^-1 w, w = A^T b - z + rho x, is a dense product with an explicit
// inverse the caller built once per solve, in one of two forms:
//   direct    y+ = Kn w, Kn = (rho I + A^T A)^-1 (n x n): one pass over Kn, one over A (A @ x+);
//   Woodbury  y+ = (w - A^T K (A w)) / rho, K = (rho I + A A^T)^-1 (m x m), with
//             A w = A A^T b - A z + rho A x from the batched pass A @ [x+ | z+]: one pass over K and
//             two over A, the dual solver's schedule.
// The row step (k_admm_primal) updates x, y, z in place and writes the next w; one record is read
// back per iteration, as in admm.cpp (both Gram matrices are of n x l iterates here).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "glx_host.h"

namespace glx {
namespace {

using namespace split;

void check_opts(const glx_admm_primal_opts* o) {
  if (!o) throw Error{GLX_E_INVALID, "null opts"};
  if (o->maxit < 0 || o->max_total_iters < 0) throw Error{GLX_E_INVALID, "negative iteration limit"};
  if (o->form < 0 || o->form > 2) throw Error{GLX_E_INVALID, "form must be 0 (auto), 1 (direct) or 2 (Woodbury)"};
  if (!(o->rho > 0.0)) throw Error{GLX_E_INVALID, "rho must be positive"};
  if (!(o->eta_0 > 0.0)) throw Error{GLX_E_INVALID, "eta_0 must be positive"};
  if (o->step_type != GLX_STEP_FIXED && o->step_type != GLX_STEP_DIMINISHING && o->step_type != GLX_STEP_DIMINISHING2)
    throw Error{GLX_E_INVALID, "step_type must be fixed, diminishing or diminishing2"};
}

// opts.form: 0 auto = Woodbury exactly when m^2 + m n < n^2: the bytes an iteration streams,
// 2 m n + m^2 (Woodbury) against n^2 + m n (direct). A byte count, not a measurement (DESIGN.md,
// "Primal ADMM").
bool use_woodbury(int form, int64_t m, int64_t n) {
  if (form != 0) return form == 2;
  const double dm = (double)m, dn = (double)n;
  return dm * dm + dm * dn < dn * dn;
}

// The launch plans of a solve: A's is the dual solver's (glx_host.h a_plan); the inverse's is the
// planner's choice for a square matrix, m x m (Woodbury's K) or n x n (direct's Kn).
struct PrimalPlan {
  int es = 8;
  bool woodbury = false;
  GemmPlan a{}, k{};
};
PrimalPlan primal_plan(int dtype, int64_t m, int64_t n, int64_t l, int form) {
  check_dtype(dtype);
  if (m <= 0 || n <= 0 || l <= 0) throw Error{GLX_E_INVALID, "m, n, l must be positive"};
  if (l > split::kMaxL) throw Error{GLX_E_INVALID, "the primal ADMM solver takes l <= 32"};
  PrimalPlan p;
  p.es = dtype == GLX_F64 ? 8 : 4;
  p.woodbury = use_woodbury(form, m, n);
  if (dtype == GLX_F32 && (m < n || p.woodbury))
    throw Error{GLX_E_INVALID,
                "the primal ADMM solver takes fp32 only for m >= n in the direct form: the conditioning of "
                "rho I + A^T A (||A||^2 / rho, 1e5 .. 1e6 at the default rho for m < n) is beyond an fp32 "
                "inverse and fp32 iterates, which never meet the stop rule; use fp64"};
  p.a = a_plan(dtype, m, n, l);
  p.k = p.woodbury ? make_plan(p.es, m, m, l, 0) : make_plan(p.es, n, n, l, 0);
  return p;
}
// slabs of the pass over A: the batched A @ [x | z] (Woodbury) or A @ x (direct)
int a_split(const PrimalPlan& p) { return ax_split(p.a, p.woodbury ? 2 : 1); }

std::string describe_primal(const PrimalPlan& p) {
  if (p.woodbury)
    return "form=Woodbury; K v=" + plan_field(p.k, 0) + "; A^T q=" + plan_field(p.a, 3) + "; A [x|z]=" +
           plan_field(p.a, 1) + "; row step=k_admm_primal";
  return "form=direct; Kn w=" + plan_field(p.k, 0) + "; A x=" + plan_field(p.a, 0) + "; row step=k_admm_primal";
}

struct PrimalWs {
  double* part; unsigned* ticket; double* gram_part; double* rec;
  void *y, *z, *w, *r, *s, *Ax, *Az, *v, *q, *pa, *pk, *gp;
};
size_t primal_carve(const PrimalPlan& p, int64_t m, int64_t n, int64_t l, void* base, PrimalWs* out) {
  Carver c(base);
  const size_t es = (size_t)p.es;
  PrimalWs w;
  std::memset(&w, 0, sizeof w);
  w.part = static_cast<double*>(c.take(sizeof(double) * kMaxRedVals * kMaxBlocks));
  w.ticket = static_cast<unsigned*>(c.take(kTicketBytes));
  w.gram_part = static_cast<double*>(c.take(sizeof(double) * 256 * l * l));
  w.rec = static_cast<double*>(c.take(sizeof(double) * (kRecHead + 2 * l * l)));
  w.y = c.take(es * n * l);
  w.z = c.take(es * n * l);
  w.w = c.take(es * n * l);
  w.r = c.take(es * n * l);
  w.s = c.take(es * n * l);
  w.Ax = c.take(es * m * l);
  w.pa = c.take(es * m * l * (p.woodbury ? 2 : 1) * std::max(1, a_split(p)));
  if (p.woodbury) {
    w.Az = c.take(es * m * l);
    w.v = c.take(es * m * l);
    w.q = c.take(es * m * l);
    w.pk = c.take(es * m * l * std::max(1, p.k.ax_S));
    w.gp = c.take(es * n * l * std::max(1, p.a.atr_S));   // the K-split slabs of A^T q
  } else {
    w.pk = c.take(es * n * l * std::max(1, p.k.ax_S));   // the K-split slabs of Kn w
  }
  if (out) *out = w;
  return c.off + 256;
}

double step_eta(const glx_admm_primal_opts& O, int64_t k) {   // set_step (:67-73), k already incremented
  if (O.step_type == GLX_STEP_DIMINISHING) return O.eta_0 / std::sqrt((double)k);
  if (O.step_type == GLX_STEP_DIMINISHING2) return O.eta_0 / (double)k;
  return O.eta_0;
}

template <typename T>
void primal_solve(const glx_problem& P, const T* K, const T* ATb, const T* AATb, const glx_admm_primal_opts& O,
                  void* ws, size_t wsb, glx_result* res, hipStream_t st) {
  const int64_t m = P.m, n = P.n, l = P.l, nl = n * l, ml = m * l;
  const int ll = (int)(l * l);
  const PrimalPlan pl = primal_plan(P.dtype, m, n, l, O.form);
  check_workspace(primal_carve(pl, m, n, l, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                  "glx_admm_primal_workspace_bytes");
  PrimalWs w;
  primal_carve(pl, m, n, l, ws, &w);
  const bool wb = pl.woodbury;
  const int SA = a_split(pl), SK = pl.k.ax_S, SG = pl.a.atr_S;
  const T* A = static_cast<const T*>(P.A);
  const T* b = static_cast<const T*>(P.b);
  T *x = static_cast<T*>(P.x), *y = static_cast<T*>(w.y), *z = static_cast<T*>(w.z), *wv = static_cast<T*>(w.w);
  T *r = static_cast<T*>(w.r), *s = static_cast<T*>(w.s), *Ax = static_cast<T*>(w.Ax), *Az = static_cast<T*>(w.Az);
  T *v = static_cast<T*>(w.v), *q = static_cast<T*>(w.q), *pa = static_cast<T*>(w.pa), *pk = static_cast<T*>(w.pk);
  T* gp = static_cast<T*>(w.gp);
  double* rec = w.rec;
  const double mu = P.mu0;
  SplitLoop loop(rec, l, nl, mu, O.thres, O.converge_len, res);
  int64_t maxit = O.maxit;
  if (O.max_total_iters > 0) maxit = std::min<int64_t>(maxit, O.max_total_iters);

  const auto t0 = std::chrono::steady_clock::now();
  GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
  GLX_HIP(hipMemsetAsync(rec, 0, sizeof(double) * loop.nrec, st));
  GLX_HIP(hipMemcpyAsync(y, x, sizeof(T) * nl, hipMemcpyDeviceToDevice, st));   // y = z = x0 (:53-55)
  GLX_HIP(hipMemcpyAsync(z, x, sizeof(T) * nl, hipMemcpyDeviceToDevice, st));
  auto red = [&](int slot) { return Red{w.part, w.ticket, rec + slot}; };
  auto pass_over_a = [&]() {   // Ax+, ||Ax+ - b||^2 and, for Woodbury, Az+ and v = A w+
    const T* xs[3] = {x, wb ? z : nullptr, nullptr};
    launch_ax<T>(pl.a, wb ? 2 : 1, A, xs, pa, nullptr, 0, st);
    launch_admm_primal_fin<T>(pa, SA, b, wb ? AATb : nullptr, Ax, Az, v, ml, O.rho, red(0), st);
  };
  launch_admm_primal_w<T>(ATb, x, z, wv, nl, O.rho, st);
  pass_over_a();
  launch_rownorm_max<T>(x, n, l, red(1), st);   // the objective of x0, returned when maxit = 0
  check_launch();
  int64_t ax_calls = 1, atr_calls = 0, k_calls = 0;
  int64_t k = 0;
  loop.begin();
  while (k < maxit) {
    ++k;
    const double eta = step_eta(O, k);
    const AdmmPrimalScalars sc{O.rho, eta * O.rho, eta * mu, O.tau * O.rho, O.thres};
    if (wb) {
      {   // q = K v
        const T* vs[3] = {v, nullptr, nullptr};
        launch_ax<T>(pl.k, 1, K, vs, SK > 1 ? pk : q, nullptr, 0, st);
        if (SK > 1) launch_sum_partials<T>(pk, SK, q, ml, st);
      }
      launch_atr<T>(pl.a, A, q, gp, st);   // g = A^T q, as slabs
      ++atr_calls;
      launch_admm_primal<T>(true, gp, SG, x, y, z, wv, ATb, x, y, z, r, s, wv, n, l, sc, red(1), st);
    } else {
      const T* vs[3] = {wv, nullptr, nullptr};   // Kn w, as slabs
      launch_ax<T>(pl.k, 1, K, vs, pk, nullptr, 0, st);
      launch_admm_primal<T>(false, pk, SK, x, y, z, wv, ATb, x, y, z, r, s, wv, n, l, sc, red(1), st);
    }
    ++k_calls;
    pass_over_a();
    ++ax_calls;
    launch_count_above<T>(x, nl, rec + 2, red(3), st);
    launch_gram<T>(r, n, l, w.gram_part, rec + kRecHead, st);
    launch_gram<T>(s, n, l, w.gram_part, rec + kRecHead + ll, st);
    if (loop.end_iteration(st)) break;
  }
  loop.finish(k, t0, st, /*count_maxit0_sync=*/false);
  res->ax_calls = ax_calls;
  res->ax_sources = (wb ? 2 : 1) * ax_calls;
  res->atr_calls = atr_calls;
  res->stats[0] = (double)k_calls;       // passes over the inverse
  res->stats[1] = wb ? 2.0 : 1.0;        // the resolved form
}


}  // namespace
}  // namespace glx

using namespace glx;

extern "C" {

int glx_admm_primal_default_opts(glx_admm_primal_opts* o) {
  return guarded([&] {
    if (!o) throw Error{GLX_E_INVALID, "null opts"};
    std::memset(o, 0, sizeof(*o));
    // gl_ADMM_primal.py:11-20
    o->maxit = 100;
    o->thres = 1e-3;
    o->tau = (1 + std::sqrt(5.0)) * 0.5;
    o->rho = 1e-2;
    o->eta_0 = 100.0;
    o->converge_len = 10;
    o->step_type = GLX_STEP_FIXED;
  });
}

int glx_admm_primal_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l,
                                    const glx_admm_primal_opts* opts, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (opts) check_opts(opts);
    *bytes = primal_carve(primal_plan(dtype, m, n, l, opts ? opts->form : 0), m, n, l, nullptr, nullptr);
  });
}

int glx_admm_primal_describe(int dtype, int64_t m, int64_t n, int64_t l, const glx_admm_primal_opts* opts,
                             char* out, size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    if (opts) check_opts(opts);
    std::snprintf(out, cap, "%s", describe_primal(primal_plan(dtype, m, n, l, opts ? opts->form : 0)).c_str());
  });
}

int glx_admm_primal_solve(const glx_problem* prob, const void* K_device, const void* ATb_device,
                          const void* AATb_device, const glx_admm_primal_opts* opts, void* ws, size_t wsb,
                          glx_result* res, void* stream) {
  return guarded([&] {
    if (!prob || !res) throw Error{GLX_E_INVALID, "null problem/result"};
    check_opts(opts);
    if (prob->comm != nullptr) throw Error{GLX_E_INVALID, "the primal ADMM solver is single-GPU: comm must be NULL"};
    if (!prob->A || !prob->b || !prob->x) throw Error{GLX_E_INVALID, "A, b and x must be device pointers"};
    if (!K_device) throw Error{GLX_E_INVALID, "K (the inverse of rho I + A^T A, or of rho I + A A^T) must be a device pointer"};
    if (!ATb_device) throw Error{GLX_E_INVALID, "ATb (A^T b) must be a device pointer"};
    const PrimalPlan pl = primal_plan(prob->dtype, prob->m, prob->n, prob->l, opts->form);   // dtype, shape, fp32 rule
    if (pl.woodbury && !AATb_device) throw Error{GLX_E_INVALID, "the Woodbury form needs AATb (A A^T b)"};
    if ((reinterpret_cast<uintptr_t>(prob->A) | reinterpret_cast<uintptr_t>(prob->b) |
         reinterpret_cast<uintptr_t>(prob->x) | reinterpret_cast<uintptr_t>(K_device) |
         reinterpret_cast<uintptr_t>(ATb_device) | (pl.woodbury ? reinterpret_cast<uintptr_t>(AATb_device) : 0)) & 15)
      throw Error{GLX_E_INVALID, "A, b, x, K, ATb, AATb must be 16-byte aligned"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(prob->dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      primal_solve<T>(*prob, static_cast<const T*>(K_device), static_cast<const T*>(ATb_device),
                      static_cast<const T*>(AATb_device), *opts, ws, wsb, res, st);
    });
  });
}

int glx_admm_primal_step(int dtype, int64_t n, int64_t l, int form, int S, const void* prod, const void* x,
                         const void* y, const void* z, const void* w, const void* ATb, double rho, double tau,
                         double eta, double mu, double thres, void* x_out, void* y_out, void* z_out,
                         void* r_out, void* s_out, void* w_out, void* sums_dev, void* ws, size_t wsb,
                         void* stream) {
  return guarded([&] {
    check_dtype(dtype);
    if (n <= 0 || l <= 0 || l > split::kMaxL) throw Error{GLX_E_INVALID, "needs n > 0 and 1 <= l <= 32"};
    if (form != 1 && form != 2) throw Error{GLX_E_INVALID, "form must be 1 (direct) or 2 (Woodbury)"};
    if (S < 1) throw Error{GLX_E_INVALID, "needs S >= 1 slabs"};
    if (!prod || !x || !y || !z || !ATb || !x_out || !y_out || !z_out || !r_out || !s_out || !w_out || !sums_dev)
      throw Error{GLX_E_INVALID, "null argument"};
    if (form == 2 && !w) throw Error{GLX_E_INVALID, "the Woodbury form reads w"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Red red = glue_red(ws, wsb, sums_dev, st);
    const AdmmPrimalScalars sc{rho, eta * rho, eta * mu, tau * rho, thres};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_admm_primal<T>(form == 2, (const T*)prod, S, (const T*)x, (const T*)y, (const T*)z, (const T*)w,
                            (const T*)ATb, (T*)x_out, (T*)y_out, (T*)z_out, (T*)r_out, (T*)s_out, (T*)w_out, n,
                            l, sc, red, st);
    });
    check_launch();
  });
}

int glx_admm_primal_rhs(int dtype, int64_t nl, const void* ATb, const void* x, const void* z, double rho,
                        void* w_out, void* stream) {
  return guarded([&] {
    check_glue(dtype, nl, 1);
    if (!ATb || !x || !z || !w_out) throw Error{GLX_E_INVALID, "null argument"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_admm_primal_w<T>((const T*)ATb, (const T*)x, (const T*)z, (T*)w_out, nl, rho, st);
    });
    check_launch();
  });
}

int glx_admm_primal_fin(int dtype, int64_t ml, int S, const void* P, const void* b, const void* AATb, double rho,
                        void* Ax, void* Az, void* v, void* sums_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_glue(dtype, ml, S);
    if (!P || !b || !Ax || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    if (AATb && (!Az || !v)) throw Error{GLX_E_INVALID, "the Woodbury half (AATb given) writes Az and v"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Red red = glue_red(ws, wsb, sums_dev, st);
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_admm_primal_fin<T>((const T*)P, S, (const T*)b, (const T*)AATb, (T*)Ax, (T*)Az, (T*)v, ml, rho, red, st);
    });
    check_launch();
  });
}

}  // extern "C"
