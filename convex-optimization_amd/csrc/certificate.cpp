// certificate.cpp — the native driver of the optimality certificate (DESIGN.md "Certificate"): for
// any iterate x of  P(x) = 1/2 ||A x - b||_F^2 + mu sum_i ||x_i||_2  one pass over A (r = A x - b
// with ||r||^2 and <r, b>) and one over A^T (g = A^T r with the row terms of cert_row in its
// epilogue where the plan fuses, a row kernel behind launch_atr elsewhere), then one readback of an
// eight-value record from which the host composes the primal and dual objectives, the duality gap
// of the rescaled residual theta = s r, s = min(1, mu / max_i ||g_i||), and the KKT violation.
// Single GPU; beside the solvers' drivers and independent of Session<T>.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "glx_host.h"

namespace glx {
namespace {

constexpr int kCertRec = 8;   // the record: [||r||^2, <r, b>] (k_cert_fin), the five row sums, fused

// A's plan and its fuse condition are glx_host.h's (fuse_plan), behind the certificate's own checks
FusePlan cert_plan(int dtype, int64_t m, int64_t n, int64_t l) {
  check_dtype(dtype);
  if (m <= 0 || n <= 0 || l <= 0) throw Error{GLX_E_INVALID, "m, n, l must be positive"};
  if (l > kMaxL) throw Error{GLX_E_INVALID, "the certificate takes l <= 128"};
  return fuse_plan(dtype, m, n, l);
}
void check_fused(int fused) {
  if (fused < 0 || fused > 2) throw Error{GLX_E_INVALID, "fused must be 0 (auto), 1 (on) or 2 (off)"};
}
// fused: 0 auto, 1 on (where admitted), 2 off. Auto = on (DESIGN.md "Certificate": the A/B).
bool use_fused(const FusePlan& p, int fused) { return p.fuse_ok && fused != 2; }

std::string describe_cert(const FusePlan& p, int fused) {
  std::string s = "A x=" + plan_field(p.a, 0) + "; A^T r=" + plan_field(p.a, 3) + "; rows=";
  s += use_fused(p, fused) ? "fused (k_atr_cert, the A^T r epilogue)"
                           : (p.fuse_ok ? "row kernel (k_cert_panel, the epilogue's layout)" : "row kernel (k_cert_row)");
  return s;
}

struct CertWs {
  double* part; unsigned* ticket; unsigned* pcnt; double* rec;
  void *r, *pa, *gp;
};
size_t cert_carve(const FusePlan& p, int64_t m, int64_t n, int64_t l, void* base, CertWs* out) {
  Carver c(base);
  const size_t es = (size_t)p.es;
  CertWs w;
  w.part = static_cast<double*>(c.take(sizeof(double) * kMaxRedVals * kMaxBlocks));
  w.ticket = static_cast<unsigned*>(c.take(kTicketBytes));
  w.pcnt = static_cast<unsigned*>(c.take(sizeof(unsigned) * (n / 64 + 64)));
  w.rec = static_cast<double*>(c.take(sizeof(double) * kCertRec));
  w.r = c.take(es * m * l);
  w.pa = c.take(es * m * l * std::max(1, ax_split(p.a, 1)));
  w.gp = c.take(es * n * l * std::max(1, p.a.atr_S));   // the K-split slabs of A^T r
  if (out) *out = w;
  return c.off + 256;
}
void check_ws(const FusePlan& pl, int64_t m, int64_t n, int64_t l, const void* ws, size_t wsb) {
  check_workspace(cert_carve(pl, m, n, l, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_certificate_workspace_bytes");
}

// the A^T pass and the row terms: g = A^T R, the five sums into red
template <typename T>
void cert_rows(const FusePlan& pl, bool fused, const T* A, const T* R, const T* x, double mu, T* G, double* rn,
               const CertWs& w, Red red, hipStream_t st) {
  const int SG = pl.a.atr_S;
  T* gp = static_cast<T*>(w.gp);
  if (fused) {
    launch_atr_cert<T>(pl.a, A, R, G, x, rn, mu, red, st, SG > 1 ? gp : nullptr, w.pcnt);
    return;
  }
  // the row kernel on the slabs: where the plan would fuse, on the epilogue's panel layout, so
  // that fused = 1 and fused = 2 give the same bits (the sums' order included)
  launch_atr<T>(pl.a, A, R, gp, st);
  if (pl.fuse_ok) launch_cert_panel<T>(pl.a, x, gp, SG, G, rn, mu, red, st);
  else launch_cert_row<T>(x, gp, SG, G, rn, pl.a.n, pl.a.l, mu, red, st);
}

template <typename T>
void certificate(const FusePlan& pl, int64_t m, int64_t n, int64_t l, const T* A, const T* X, const T* b,
                 double mu, int fused_opt, T* G, double* rn, double* out, void* ws, hipStream_t st,
                 const GroupView* grp, const SampleView* sw, double* holdout_sum, const InterceptView* ic) {
  CertWs w;
  cert_carve(pl, m, n, l, ws, &w);
  const bool fused = grp == nullptr && use_fused(pl, fused_opt);
  const int64_t ml = m * l;
  T *r = static_cast<T*>(w.r), *pa = static_cast<T*>(w.pa);
  GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
  GLX_HIP(hipMemsetAsync(w.pcnt, 0, sizeof(unsigned) * (n / 64 + 64), st));
  GLX_HIP(hipMemsetAsync(w.rec, 0, sizeof(double) * kCertRec, st));
  const T* xs[3] = {X, nullptr, nullptr};
  launch_ax<T>(pl.a, 1, A, xs, pa, nullptr, 0, st);
  const bool hold = sw != nullptr && sw->hold != nullptr;
  if (ic != nullptr) {
    // the intercept eliminated: r^ and its weighted column means, then r = w (r^ - 1 mean^T), the
    // operand of the A^T pass, and the sums on the centred residual (DESIGN.md "Intercept")
    const T* wv = sw != nullptr ? static_cast<const T*>(sw->w) : nullptr;
    T* rh = static_cast<T*>(ic->rhat);
    GLX_HIP(hipMemsetAsync(ic->cnt, 0, 256, st));
    launch_cert_csum<T>(pa, ax_split(pl.a, 1), b, wv, rh, m, l, ic->sigma, ic->part, ic->cnt, ic->mean, st);
    launch_cert_fin_c<T>(rh, b, wv, hold ? static_cast<const T*>(sw->hold) : nullptr, ic->mean, nullptr, r, ml, l,
                         Red{w.part, w.ticket, hold ? sw->sums : w.rec}, st);
  } else if (sw != nullptr) {
    // r = w (A x - b), the operand of the A^T pass. Two sums go where k_cert_fin's go; with hold-out
    // weights there are three, which rec + 2 has no room for: they go to sw->sums
    launch_cert_fin_w<T>(pa, ax_split(pl.a, 1), b, static_cast<const T*>(sw->w), static_cast<const T*>(sw->hold),
                         nullptr, r, ml, l, Red{w.part, w.ticket, hold ? sw->sums : w.rec}, st);
  } else {
    launch_cert_fin<T>(pa, ax_split(pl.a, 1), b, r, ml, Red{w.part, w.ticket, w.rec}, st);
  }
  const bool sgl = grp != nullptr && grp->row_ratio > 0.0;
  if (sgl) {
    // the sparse-group terms (DESIGN.md "Sparse-group lasso"): the row norms and six sums, then the two
    // dual solves on the row norms. rec[8], rec[9] lie in the record's own 256-byte piece of the workspace
    const double tau = grp->row_ratio;
    double* rho = rn != nullptr ? rn : grp->rho;
    if (rho == nullptr) throw Error{GLX_E_INVALID, "sparse-group certificate: no room for the row norms"};
    launch_atr<T>(pl.a, A, r, static_cast<T*>(w.gp), st);
    launch_sgl_cert<T>(X, static_cast<const T*>(w.gp), pl.a.atr_S, G, rho, grp->ptr, grp->wts, grp->G, n, l, mu, tau,
                       Red{w.part, w.ticket, w.rec + 2}, st);
    launch_sgl_dual_scale(rho, grp->ptr, grp->wts, grp->G, tau * mu, (1.0 - tau) * mu, 1.0, 0.0, grp->pad_mul,
                          grp->pad_add, hold ? sw->sums : w.rec, nullptr, Red{w.part, w.ticket, w.rec + 8}, st);
  } else if (grp != nullptr) {   // the group terms on the slabs of the plain product
    launch_atr<T>(pl.a, A, r, static_cast<T*>(w.gp), st);
    launch_group_cert<T>(X, static_cast<const T*>(w.gp), pl.a.atr_S, G, rn, grp->ptr, grp->wts, grp->G, n, l,
                         grp->max_run, mu, Red{w.part, w.ticket, w.rec + 2}, st);
  } else {
    cert_rows<T>(pl, fused, A, r, X, mu, G, rn, w, Red{w.part, w.ticket, w.rec + 2}, st);
  }
  check_launch();
  double hs[3] = {0.0, 0.0, 0.0};
  GLX_HIP(hipMemcpyAsync(out, w.rec, sizeof(double) * kCertRec, hipMemcpyDeviceToHost, st));
  double sd[2] = {0.0, 0.0};
  if (sgl) GLX_HIP(hipMemcpyAsync(sd, w.rec + 8, sizeof sd, hipMemcpyDeviceToHost, st));
  if (hold) GLX_HIP(hipMemcpyAsync(hs, sw->sums, sizeof hs, hipMemcpyDeviceToHost, st));
  if (ic != nullptr)
    GLX_HIP(hipMemcpyAsync(ic->mean_host, ic->mean, sizeof(double) * l, hipMemcpyDeviceToHost, st));
  GLX_HIP(hipStreamSynchronize(st));
  if (sgl) {
    // the record in compose's terms: out[3] = mu / s with s = min_g s_g, nudged up so that the mu / out[3]
    // compose forms is at most s (s = +inf: 0; s <= 0: +inf); out[7] = the nonzero rows
    const double s0 = -sd[0], s1 = -sd[1], rmax = out[3];
    double ge = s0 > 0.0 ? mu / s0 : (s0 <= 0.0 ? std::numeric_limits<double>::infinity() : s0);
    for (int k = 0; k < 4 && ge > 0.0 && std::isfinite(ge) && mu / ge > s0; ++k)
      ge = std::nextafter(ge, std::numeric_limits<double>::infinity());
    out[3] = ge;
    if (grp->extra != nullptr) {
      grp->extra[0] = s0;
      grp->extra[1] = s1;
      grp->extra[2] = rmax;
      grp->extra[3] = 0.0;
    }
  } else {
    out[7] = fused ? 1.0 : 0.0;
  }
  if (hold) {
    out[0] = hs[0];
    out[1] = hs[1];
  }
  if (holdout_sum != nullptr) *holdout_sum = hs[2];
}

}  // namespace

void certificate_run(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                     double mu, int fused, void* G_out, double* rownorm_out, double* out, void* ws, size_t wsb,
                     void* stream, const GroupView* grp, const SampleView* sw, double* holdout_sum,
                     const InterceptView* ic) {
  const FusePlan pl = cert_plan(dtype, m, n, l);
  check_fused(fused);
  if (sw != nullptr && (!sw->w || !sw->sums)) throw Error{GLX_E_INVALID, "sample weights: null vector or sums"};
  if (ic != nullptr) {
    check_intercept(ic->sigma, ic->mean_host);
    if (!ic->rhat || !ic->mean || !ic->part || !ic->cnt) throw Error{GLX_E_INVALID, "intercept: null workspace piece"};
  }
  if (grp != nullptr && !(grp->row_ratio >= 0.0 && grp->row_ratio <= 1.0))
    throw Error{GLX_E_INVALID, "row_ratio must be in [0, 1] (and not NaN)"};
  if (grp != nullptr && grp->row_ratio > 0.0 && ic != nullptr)
    throw Error{GLX_E_INVALID, "the sparse-group penalty (row_ratio > 0) takes no intercept"};
  if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
  if (!A || !X || !b) throw Error{GLX_E_INVALID, "A, X and b must be device pointers"};
  if (!out) throw Error{GLX_E_INVALID, "null out"};
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(b) |
       reinterpret_cast<uintptr_t>(G_out)) & 15)
    throw Error{GLX_E_INVALID, "A, X, b, G_out must be 16-byte aligned"};
  check_ws(pl, m, n, l, ws, wsb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  by_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    certificate<T>(pl, m, n, l, (const T*)A, (const T*)X, (const T*)b, mu, fused, (T*)G_out, rownorm_out, out, ws, st,
                   grp, sw, holdout_sum, ic);
  });
}

size_t intercept_carve(size_t head, int es, int64_t m, int64_t l, void* base, InterceptView* out) {
  Carver c(base);
  InterceptView v;
  c.take(head);
  v.rhat = c.take((size_t)es * (size_t)m * (size_t)l);
  v.mean = static_cast<double*>(c.take(sizeof(double) * (size_t)l));
  v.part = static_cast<double*>(c.take(cert_csum_part_bytes()));
  v.cnt = static_cast<unsigned*>(c.take(256));
  if (out) {
    out->rhat = v.rhat;
    out->mean = v.mean;
    out->part = v.part;
    out->cnt = v.cnt;
  }
  return c.off + 256;
}

void check_intercept(double weight_sum, const double* intercept_out) {
  if (!(weight_sum > 0.0) || !std::isfinite(weight_sum))
    throw Error{GLX_E_INVALID, "intercept: weight_sum must be positive and finite"};
  if (!intercept_out) throw Error{GLX_E_INVALID, "intercept: null intercept_out"};
}

void check_sample(const void* sample_w, const void* holdout_w) {
  if (holdout_w != nullptr && sample_w == nullptr)
    throw Error{GLX_E_INVALID, "holdout_w goes with sample_w (pass ones for an unweighted fit)"};
  if ((reinterpret_cast<uintptr_t>(sample_w) | reinterpret_cast<uintptr_t>(holdout_w)) & 15)
    throw Error{GLX_E_INVALID, "sample_w and holdout_w must be 16-byte aligned"};
}

}  // namespace glx

using namespace glx;

extern "C" {

int glx_certificate_sw_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    *bytes = sample_bytes(cert_carve(cert_plan(dtype, m, n, l), m, n, l, nullptr, nullptr));
  });
}

int glx_certificate_sw_describe(int dtype, int64_t m, int64_t n, int64_t l, int fused, char* out, size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    check_fused(fused);
    std::snprintf(out, cap, "%s; residual=weighted finalize (k_cert_fin_w)",
                  describe_cert(cert_plan(dtype, m, n, l), fused).c_str());
  });
}

int glx_certificate_sw(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                       double mu, int fused, const void* sample_w, const void* holdout_w, void* G_out,
                       double* rownorm_out, double* out, double* holdout_sum, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_sample(sample_w, holdout_w);
    const size_t head = cert_carve(cert_plan(dtype, m, n, l), m, n, l, nullptr, nullptr);
    if (!ws) throw Error{GLX_E_INVALID, "null workspace"};   // (the alignment: certificate_run's check, below)
    if (wsb < sample_bytes(head))
      throw Error{GLX_E_INVALID, "workspace too small (glx_certificate_sw_workspace_bytes)"};
    if (holdout_sum != nullptr) *holdout_sum = 0.0;
    if (sample_w == nullptr) {   // today's entry, call for call
      certificate_run(dtype, m, n, l, A, X, b, mu, fused, G_out, rownorm_out, out, ws, head, stream, nullptr);
      return;
    }
    SampleView sw;
    sw.w = sample_w;
    sw.hold = holdout_w;
    sw.sums = reinterpret_cast<double*>(static_cast<char*>(ws) + sample_off(head));
    certificate_run(dtype, m, n, l, A, X, b, mu, fused, G_out, rownorm_out, out, ws, head, stream, nullptr, &sw,
                    holdout_sum);
  });
}

/* ---- the unpenalised intercept (DESIGN.md "Intercept"): [the _sw entry's workspace | the centring
 * finalize's pieces] ---- */

int glx_certificate_ic_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    const FusePlan pl = cert_plan(dtype, m, n, l);
    *bytes = intercept_carve(sample_bytes(cert_carve(pl, m, n, l, nullptr, nullptr)), pl.es, m, l, nullptr, nullptr);
  });
}

int glx_certificate_ic_describe(int dtype, int64_t m, int64_t n, int64_t l, int fused, char* out, size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    check_fused(fused);
    std::snprintf(out, cap, "%s; residual=centring finalize (k_cert_csum, k_cert_fin_c)",
                  describe_cert(cert_plan(dtype, m, n, l), fused).c_str());
  });
}

int glx_certificate_ic(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                       double mu, int fused, const void* sample_w, const void* holdout_w, double weight_sum,
                       void* G_out, double* rownorm_out, double* out, double* holdout_sum, double* intercept_out,
                       void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_sample(sample_w, holdout_w);
    check_intercept(weight_sum, intercept_out);
    const FusePlan pl = cert_plan(dtype, m, n, l);
    const size_t head = cert_carve(pl, m, n, l, nullptr, nullptr);
    check_workspace(intercept_carve(sample_bytes(head), pl.es, m, l, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                    "glx_certificate_ic_workspace_bytes");
    if (holdout_sum != nullptr) *holdout_sum = 0.0;
    InterceptView ic;
    ic.sigma = weight_sum;
    ic.mean_host = intercept_out;
    intercept_carve(sample_bytes(head), pl.es, m, l, ws, &ic);
    SampleView sw;
    sw.w = sample_w;
    sw.hold = holdout_w;
    sw.sums = reinterpret_cast<double*>(static_cast<char*>(ws) + sample_off(head));
    certificate_run(dtype, m, n, l, A, X, b, mu, fused, G_out, rownorm_out, out, ws, head, stream, nullptr,
                    sample_w != nullptr ? &sw : nullptr, holdout_sum, &ic);
    for (int64_t c = 0; c < l; ++c) intercept_out[c] = -intercept_out[c];   // c = -r-bar
  });
}

int glx_certificate_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    *bytes = cert_carve(cert_plan(dtype, m, n, l), m, n, l, nullptr, nullptr);
  });
}

int glx_certificate_describe(int dtype, int64_t m, int64_t n, int64_t l, int fused, char* out, size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    check_fused(fused);
    std::snprintf(out, cap, "%s", describe_cert(cert_plan(dtype, m, n, l), fused).c_str());
  });
}

int glx_certificate(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                    double mu, int fused, void* G_out, double* rownorm_out, double* out, void* ws, size_t wsb,
                    void* stream) {
  return guarded([&] {
    certificate_run(dtype, m, n, l, A, X, b, mu, fused, G_out, rownorm_out, out, ws, wsb, stream, nullptr);
  });
}

int glx_certificate_step(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* Z, void* G,
                         const void* x, double mu, int form, double* rownorm_out, void* sums_dev, void* ws,
                         size_t wsb, void* stream) {
  return guarded([&] {
    if (form != 0 && form != 1) throw Error{GLX_E_INVALID, "form must be 0 (row kernel) or 1 (A^T r epilogue)"};
    const FusePlan pl = cert_plan(dtype, m, n, l);
    if (!G || !x || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    if (form == 1) {
      if (!A || !Z) throw Error{GLX_E_INVALID, "form 1 needs A and Z"};
      if (!pl.fuse_ok)
        throw Error{GLX_E_INVALID, "form 1: this shape's A^T R plan takes no fused epilogue (" + describe_plan(pl.a) + ")"};
    }
    check_ws(pl, m, n, l, ws, wsb);
    CertWs w;
    cert_carve(pl, m, n, l, ws, &w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    GLX_HIP(hipMemsetAsync(w.pcnt, 0, sizeof(unsigned) * (n / 64 + 64), st));
    Red red{w.part, w.ticket, static_cast<double*>(sums_dev)};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      if (form == 0 && pl.fuse_ok)   // the layout the driver's unfused arm takes at this (m, n, l)
        launch_cert_panel<T>(pl.a, (const T*)x, (const T*)G, 1, nullptr, rownorm_out, mu, red, st);
      else if (form == 0)
        launch_cert_row<T>((const T*)x, (const T*)G, 1, nullptr, rownorm_out, n, l, mu, red, st);
      else
        launch_atr_cert<T>(pl.a, (const T*)A, (const T*)Z, (T*)G, (const T*)x, rownorm_out, mu, red, st,
                           pl.a.atr_S > 1 ? (T*)w.gp : nullptr, w.pcnt);
    });
    check_launch();
  });
}

}  // extern "C"
