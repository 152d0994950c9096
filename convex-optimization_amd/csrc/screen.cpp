// screen.cpp — the native driver of the certified solve (DESIGN.md "Certified solve and screening"):
// FISTA with the exact group prox and a fixed step t <= 1 / lambda_max(A^T A) on
//   P(x) = 1/2 ||A x - b||_F^2 + mu sum_i ||x_i||_2,
// stopped on the certificate's relative duality gap, with gap-safe screening: every check_every
// iterations the certificate of the current (reduced) problem gives a dual point theta = s r and
// the radius rho = sqrt(2 gap) of a ball that holds the dual optimum; a row with
// s ||g_i|| + ||a_i|| rho < mu is zero at the optimum, and its column leaves A. The radius carries a
// rounding guard composed on the host in float64 (glx_screen_guard). Kept columns are gathered into
// one of two workspace buffers, padded with zero columns to a multiple of 64 so that the reduced
// problem keeps the MFMA A^T r panel. One iteration is launch_ax on y, the residual finalize, and
// the FISTA epilogue of A^T r (launch_atr_fista) or, where the plan does not fuse, launch_atr and the
// row kernel (launch_fista_trial); thres is the dtype's smallest normal number, with which
// fista_row's denominator switch and hard threshold are no-ops. Single GPU; beside certificate.cpp.
// The same loop solves the grouped problem mu sum_g w_g ||x_[g]||_F (DESIGN.md "Feature groups and
// weights"; entries in group.cpp): with a GroupView the step is launch_atr + launch_group_fista, the
// certificate takes the view, the screen runs on the G "rows" ||g_[g]|| / w_g against
// ||A_[g]||_F / w_g under group_screen_guard, and launch_group_expand turns the kept groups into the
// row list a compaction gathers with. Without a view every call and every byte is the row solve's.
// With a SampleView (DESIGN.md "Sample weights and cross-validation") the loop solves
// 1/2 sum_j w_j ||(A x - b)_j||^2 + mu Omega(x): the two residual finalizes become launch_cert_fin_w
// (r = w (A y - b) is the R every step already takes), ||b~|| and the column figures are the weighted
// ones, every certificate takes the weights and the guards count their roundings; the final
// certificate also reduces the hold-out sum. Without one, again, nothing differs.
// A GroupView with row_ratio > 0 (DESIGN.md "Sparse-group lasso") adds a row term to the group penalty:
// the step is launch_atr + launch_sgl_fista, the certificate takes the view (its dual scaling is a
// per-group solve, done twice: plain, and on the row norms padded by sgl_guard_pad), the screen is
// launch_sgl_screen on rows and groups under sgl_screen_guard and launch_sgl_expand turns its row flags
// into the row list and the reduced groups. It composes with a SampleView and refuses an InterceptView.
// With an InterceptView (DESIGN.md "Intercept") the loop solves min_c 1/2 sum_j w_j ||(A x + 1 c^T - b)_j||^2
// + mu Omega(x) with c eliminated exactly: the residual finalizes become the two centring launches
// (launch_cert_csum, launch_cert_fin_c: r = w (A y - b - 1 mean^T)), the column figures are the centred
// ones, every certificate centres and the screen runs under screen_guard_ic with its slack off mu.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "glx_host.h"

namespace glx {

// gamma_k = k u / (1 - k u): the bar of a k-term dot product in unit roundoff u (infinite once
// k u >= 1, which switches screening off)
double gamma_k(double k, double u) {
  const double ku = k * u;
  return ku < 1.0 ? ku / (1.0 - ku) : std::numeric_limits<double>::infinity();
}

namespace {

inline int64_t pad64(int64_t v) { return (v + 63) / 64 * 64; }

// The rounding guard (DESIGN.md "Certified solve and screening", "The guard, term by term").
// rec: the certificate's record of the stored residual r^ and g^ = A^T r^ in dtype arithmetic.
// out = [s_safe, gap+, rho+]. Every quantity below is an upper bound; NaN propagates (and then
// keeps every row in k_screen).
// weighted: the sample-weighted problem's record and figures (cmax, csq of the weighted column norms,
// bn = ||b~||); k counts the one more rounding of w r^ before the A^T pass, of (w r^) r^ and (w r^) b in
// the fp64 sums, and of (w a) a in the column norms (DESIGN.md "Sample weights and cross-validation").
void screen_guard(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l, double cmax,
                  double csq, double bn_in, double* out, bool weighted = false) {
  const double k = weighted ? 3.0 : 2.0;
  const double u = dtype == GLX_F64 ? DBL_EPSILON : (double)FLT_EPSILON;   // eps of A's dtype
  const double u64 = DBL_EPSILON;
  const double rr = rec[0], rb = rec[1], sx = rec[2], gmax = rec[3];
  const double rn = std::sqrt(rr);
  const double gm = gamma_k((double)m + k, u), gn = gamma_k((double)n + 2.0, u);
  const double ml = (double)m * (double)l;
  const double g_ml = gamma_k(ml + k, u64);
  const double bn = weighted ? bn_in * (1.0 + g_ml) : bn_in;   // (the weighted ||b~|| is itself such a sum)
  // 1. dual feasibility: ||a_i^T r^|| <= ||g^_i|| + gm ||a_i|| ||r^||
  const double den = gmax + gm * cmax * rn;
  const double s = den > mu ? mu / den : (den <= mu ? 1.0 : den);   // (NaN den: NaN)
  // 2. the primal value: ||r^ - (A x - b)|| <= dr
  const double dr = gn * std::sqrt(csq) * sx + u * (rn + 2.0 * bn);
  const double bar_rr = g_ml * rr;                      // the fp64 sum ||r^||^2
  const double bar_rb = g_ml * rn * bn;                 // the fp64 sum <r^, b> (Cauchy-Schwarz on sum |r b|)
  const double bar_sx = (gamma_k((double)l + 2.0, u) + gamma_k((double)n + 2.0, u64)) * sx;   // sum_i ||x_i||
  const double gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * sx;
  const double bars = rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx;
  const double gap_p = (gap > 0.0 ? gap : (gap <= 0.0 ? 0.0 : gap)) + bars;
  // 3. the row's own value: s ||a_i^T r^|| <= s ||g^_i|| (1 + gl) + s gm ||a_i|| ||r^||, and
  //    ||g^_i|| <= (1 + gm) ||a_i|| ||r^||, so both terms are ||a_i|| times a radius; the column
  //    norms themselves are low by at most gamma64_{m+2}
  const double gl = gamma_k((double)l + 2.0, u);
  double rho = std::sqrt(2.0 * gap_p) + s * gm * rn + s * gl * (1.0 + gm) * rn;
  rho *= 1.0 + gamma_k((double)m + k, u64);
  out[0] = s;
  out[1] = gap_p;
  out[2] = rho;
}

// the plan of a (reduced) problem is the certificate's: glx_host.h fuse_plan
void check_shape(int dtype, int64_t m, int64_t n, int64_t l) {
  check_dtype(dtype);
  if (m <= 0 || n <= 0 || l <= 0) throw Error{GLX_E_INVALID, "m, n, l must be positive"};
  if (l > kMaxL) throw Error{GLX_E_INVALID, "the certified solve takes l <= 128"};
  if (n > (int64_t)0x7fffffc0) throw Error{GLX_E_INVALID, "the certified solve takes n < 2^31 - 64"};
}

// the largest padded widths the two compaction buffers can be asked to hold
int64_t buf_width(int64_t w) { return (w * 9 / 10) / 64 * 64; }

// What the reduced problems need at most: over n itself and every multiple of 64 a compaction can
// reach (<= 0.9 n), the certificate's workspace and the K splits of the two products.
struct Extent {
  size_t cert = 0;
  int ax_s = 1, atr_s = 1;
};
Extent extent(int dtype, int64_t m, int64_t n, int64_t l, bool screen) {
  Extent e;
  auto take = [&](int64_t w) {
    size_t b = 0;
    if (glx_certificate_workspace_bytes(dtype, m, w, l, &b) != GLX_OK) throw Error{GLX_E_INVALID, g_last_error};
    e.cert = std::max(e.cert, b);
    const FusePlan p = fuse_plan(dtype, m, w, l);
    e.ax_s = std::max(e.ax_s, std::max(1, ax_split(p.a, 1)));
    e.atr_s = std::max(e.atr_s, std::max(1, p.a.atr_S));
  };
  take(n);
  if (screen)
    for (int64_t w = 64; w <= buf_width(n); w += 64) take(w);
  return e;
}

constexpr int kRedOut = 16;

struct Ws {
  double* part; unsigned* ticket; unsigned* pcnt; double* red;
  void* cert;
  void *r, *pa, *gp, *g, *x[5];
  double *rn, *cn[2], *cpart;
  unsigned* ccnt;
  int *map[2], *list, *cnt;
  unsigned long long* bal;
  unsigned* sticket;
  void* abuf[2];
  size_t cert_bytes;
  int64_t cap[2];
  // groups (G > 0): the two reduced descriptions a compaction alternates between, the full
  // problem's gcn, and the screen's list of kept groups
  int *gptr[2], *gmap[2], *glist;
  double *gw[2], *ggcn[2], *gcn_full;
  double* ssums;   // sample weights: the weighted finalize's sums of a certificate (SampleView::sums)
  InterceptView ic;   // intercept: the centring finalize's device pieces
  double* cmean;      // intercept: the column means of A
  int* skeep;         // sparse-group lasso: k_sgl_screen's flag per row
};
size_t carve(int dtype, int64_t m, int64_t n, int64_t l, bool screen, bool own_norms, void* base, Ws* out,
             int64_t G = 0, bool weighted = false, bool intercept = false, bool sgl = false) {
  const size_t es = dtype == GLX_F64 ? 8 : 4;
  const Extent e = extent(dtype, m, n, l, screen);
  const int64_t np = pad64(n);
  Carver c(base);
  Ws w;
  w.part = static_cast<double*>(c.take(sizeof(double) * kMaxRedVals * kMaxBlocks));
  w.ticket = static_cast<unsigned*>(c.take(kTicketBytes));
  w.pcnt = static_cast<unsigned*>(c.take(sizeof(unsigned) * (np / 64 + 64)));
  w.red = static_cast<double*>(c.take(sizeof(double) * kRedOut));
  w.cert_bytes = e.cert;
  w.cert = c.take(e.cert);
  w.r = c.take(es * m * l);
  w.pa = c.take(es * m * l * e.ax_s);
  w.gp = c.take(es * np * l * e.atr_s);
  w.g = c.take(es * np * l);
  for (int i = 0; i < 5; ++i) w.x[i] = c.take(es * np * l);
  w.rn = static_cast<double*>(c.take(sizeof(double) * np));
  for (int i = 0; i < 2; ++i) w.cn[i] = static_cast<double*>(c.take(sizeof(double) * np));
  w.cpart = static_cast<double*>(c.take(own_norms ? col_norms_part_bytes(m, n) : 0));
  w.ccnt = static_cast<unsigned*>(c.take(col_norms_count_bytes(n)));
  for (int i = 0; i < 2; ++i) w.map[i] = static_cast<int*>(c.take(sizeof(int) * np));
  w.list = static_cast<int*>(c.take(sizeof(int) * np));
  w.cnt = static_cast<int*>(c.take(sizeof(int) * 4));
  w.bal = static_cast<unsigned long long*>(c.take(screen_words_bytes(n)));
  w.sticket = static_cast<unsigned*>(c.take(256));
  w.cap[0] = screen ? buf_width(n) : 0;
  w.cap[1] = screen ? buf_width(w.cap[0]) : 0;
  for (int i = 0; i < 2; ++i) w.abuf[i] = c.take(es * (size_t)m * (size_t)w.cap[i]);
  for (int i = 0; i < 2; ++i) {   // (behind everything the row solve uses: its layout is unchanged)
    w.gptr[i] = static_cast<int*>(c.take(G > 0 ? sizeof(int) * (size_t)(G + 1) : 0));
    w.gmap[i] = static_cast<int*>(c.take(sizeof(int) * (size_t)G));
    w.gw[i] = static_cast<double*>(c.take(sizeof(double) * (size_t)G));
    w.ggcn[i] = static_cast<double*>(c.take(sizeof(double) * (size_t)G));
  }
  w.gcn_full = static_cast<double*>(c.take(sizeof(double) * (size_t)G));
  w.glist = static_cast<int*>(c.take(G > 0 ? sizeof(int) * (size_t)pad64(G) : 0));
  w.ssums = static_cast<double*>(c.take(weighted ? 256 : 0));   // (behind the grouped pieces in turn)
  w.cmean = nullptr;
  if (intercept) {   // (and the intercept's behind those)
    w.cmean = static_cast<double*>(c.take(sizeof(double) * np));
    c.off = intercept_carve(c.off, (int)es, m, l, base, &w.ic) - 256;
  }
  w.skeep = nullptr;
  if (sgl) w.skeep = static_cast<int*>(c.take(sizeof(int) * np));   // (behind everything else, and only then)
  if (out) *out = w;
  return c.off + 256;
}

std::string describe_certified(int dtype, int64_t m, int64_t n, int64_t l, bool screen, int64_t max_run = 0,
                               bool sgl = false) {
  const FusePlan p = fuse_plan(dtype, m, n, l);
  std::string s = "FISTA, fixed step, exact prox; A y=" + plan_field(p.a, 0) + "; A^T r=" + plan_field(p.a, 3) +
                  "; step=";
  if (sgl) s += "sparse-group kernel (k_sgl_fista, " + sgl_layout(l) + ")";
  else if (max_run > 0) s += "group kernel (k_group_fista, " + group_layout(max_run * l) + ")";
  else s += p.fuse_ok ? "fused (k_atr_fista, the A^T r epilogue)" : "row kernel (k_fista_trial)";
  s += screen ? "; screening=gap-safe, compaction to multiples of 64 at <= 0.9 of the width" : "; screening=off";
  return s;
}

struct Composed {
  double primal, dual, gap, rel, scale;
};
// glx/certificate.py compose, in the same order of operations
Composed compose(const double* rec, double mu) {
  const double rr = rec[0], rb = rec[1], sx = rec[2], gmax = rec[3];
  Composed c;
  c.scale = gmax <= mu ? 1.0 : mu / gmax;
  c.primal = 0.5 * rr + mu * sx;
  c.dual = -0.5 * c.scale * c.scale * rr - c.scale * rb;
  c.gap = c.primal - c.dual;
  c.rel = c.gap / std::max(std::fabs(c.primal), DBL_MIN);
  return c;
}

void cert_call(int dtype, int64_t m, int64_t w, int64_t l, const void* A, const void* x, const void* b, double mu,
               double* rn, double* rec, const Ws& ws, hipStream_t st, const GroupView* grp = nullptr,
               const SampleView* sw = nullptr, double* holdout_sum = nullptr, const InterceptView* ic = nullptr) {
  if (sw != nullptr || ic != nullptr) {   // the weighted problem's certificate, rows or groups; the intercept's
    certificate_run(dtype, m, w, l, A, x, b, mu, 0, nullptr, rn, rec, ws.cert, ws.cert_bytes, st, grp, sw,
                    holdout_sum, ic);
    return;
  }
  if (grp != nullptr) {   // (rn: ||g_[g]|| / w_g of the grp->G groups)
    certificate_run(dtype, m, w, l, A, x, b, mu, 0, nullptr, rn, rec, ws.cert, ws.cert_bytes, st, grp);
    return;
  }
  const int rc = glx_certificate(dtype, m, w, l, A, x, b, mu, 0, nullptr, rn, rec, ws.cert, ws.cert_bytes, st);
  if (rc != GLX_OK) throw Error{rc, "certified solve: " + g_last_error};
}

template <typename T>
void solve(int dtype, int64_t m, int64_t n, int64_t l, const T* A, const T* b, T* X, double mu, double t,
           double tol, int64_t maxit, bool screen, int check_every, const double* cn_in, const double* cstats_in,
           int32_t* kept_rows, void* wsp, glx_certified_info* info, hipStream_t st, const GroupView* grp,
           int32_t* kept_groups, int64_t* listed_groups, const SampleView* sw, double* holdout_sum,
           const InterceptView* icv) {
  Ws w;
  // the sparse-group lasso (DESIGN.md "Sparse-group lasso"): the view's row_ratio > 0
  const bool sgl = grp != nullptr && grp->row_ratio > 0.0;
  const double tau = sgl ? grp->row_ratio : 0.0;
  carve(dtype, m, n, l, screen, cn_in == nullptr, wsp, &w, grp != nullptr ? grp->G : 0,
        sw != nullptr || icv != nullptr, icv != nullptr, sgl);
  // the intercept (DESIGN.md "Intercept"): the caller's sigma and host means, this workspace's device pieces
  InterceptView icw = w.ic;
  if (icv != nullptr) {
    icw.sigma = icv->sigma;
    icw.mean_host = icv->mean_host;
  }
  const InterceptView* ic = icv != nullptr ? &icw : nullptr;
  double amax = 0.0, asq = 0.0;   // max |column mean| and the sum of their squares
  auto mean_sq = [&]() {          // sum_c r-bar_c^2 of the last certificate (or finalize read back)
    double q = 0.0;
    for (int64_t c = 0; c < l; ++c) q += icw.mean_host[c] * icw.mean_host[c];
    return q;
  };
  // sample weights: the loop's certificates take the weights alone, the final one the hold-out too
  const T* sww = sw != nullptr ? static_cast<const T*>(sw->w) : nullptr;
  const SampleView sw_in{sw != nullptr ? sw->w : nullptr, nullptr, w.ssums};
  const SampleView sw_out{sw != nullptr ? sw->w : nullptr, sw != nullptr ? sw->hold : nullptr, w.ssums};
  const size_t es = sizeof(T);
  const double thres = std::is_same<T, double>::value ? DBL_MIN : (double)FLT_MIN;
  const int64_t ml = m * l;
  std::memset(info, 0, sizeof *info);
  const auto t_begin = std::chrono::steady_clock::now();

  GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
  GLX_HIP(hipMemsetAsync(w.pcnt, 0, sizeof(unsigned) * (pad64(n) / 64 + 64), st));
  GLX_HIP(hipMemsetAsync(w.ccnt, 0, col_norms_count_bytes(n), st));
  GLX_HIP(hipMemsetAsync(w.sticket, 0, 256, st));
  GLX_HIP(hipMemsetAsync(w.red, 0, sizeof(double) * kRedOut, st));
  if (ic != nullptr) GLX_HIP(hipMemsetAsync(ic->cnt, 0, 256, st));
  const Red red0{w.part, w.ticket, w.red}, red1{w.part, w.ticket, w.red + 4}, red2{w.part, w.ticket, w.red + 10};

  // the column figures and ||b||_F (screening only)
  double cmax = 0.0, csq = 0.0, bn = 0.0, gcol_max = 0.0;
  const double* cn = nullptr;
  if (screen) {
    if (cn_in != nullptr) {
      cn = cn_in;
      cmax = cstats_in[0];
      csq = cstats_in[1];
      if (ic != nullptr) {
        amax = cstats_in[2];
        asq = cstats_in[3];
      }
    } else {
      if (ic != nullptr)
        launch_col_norms_c<T>(A, sww, ic->sigma, m, n, w.cn[1], w.cmean, w.cpart, w.ccnt,
                              Red{w.part, w.ticket, w.red + 13}, red2, st);
      else if (sww != nullptr) launch_col_norms_w<T>(A, sww, m, n, w.cn[1], w.cpart, w.ccnt, red2, st);
      else launch_col_norms<T>(A, m, n, w.cn[1], w.cpart, w.ccnt, red2, st);
      check_launch();
      cn = w.cn[1];
      info->passes += ic != nullptr ? 2.0 : 1.0;
    }
    // r = -b: red0 = [||b||^2, .] (weighted: sum w b^2 = ||b~||^2, the null product of k_cert_fin_w)
    // (intercept: the centring finalize of the null product gives ||P~ b~||^2 and -b-bar; the guard
    // takes the uncentred ||b~||^2 = ||P~ b~||^2 + sigma ||b-bar||^2)
    if (ic != nullptr) {
      GLX_HIP(hipMemsetAsync(ic->cnt, 0, 256, st));
      launch_cert_csum<T>(nullptr, 0, b, sww, static_cast<T*>(ic->rhat), m, l, ic->sigma, ic->part, ic->cnt,
                          ic->mean, st);
      launch_cert_fin_c<T>(static_cast<const T*>(ic->rhat), b, sww, nullptr, ic->mean, nullptr,
                           static_cast<T*>(w.r), ml, l, red0, st);
      GLX_HIP(hipMemcpyAsync(ic->mean_host, ic->mean, sizeof(double) * l, hipMemcpyDeviceToHost, st));
    } else if (sww != nullptr)
      launch_cert_fin_w<T>(nullptr, 0, b, sww, nullptr, nullptr, static_cast<T*>(w.r), ml, l, red0, st);
    else
      launch_cert_fin<T>(nullptr, 0, b, static_cast<T*>(w.r), ml, red0, st);
    check_launch();
    double h[6] = {};
    GLX_HIP(hipMemcpyAsync(h, w.red, sizeof(double), hipMemcpyDeviceToHost, st));
    GLX_HIP(hipMemcpyAsync(h + 1, w.red + 10, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (ic != nullptr) GLX_HIP(hipMemcpyAsync(h + 3, w.red + 13, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    GLX_HIP(hipStreamSynchronize(st));
    bn = std::sqrt(ic != nullptr ? (h[0] + ic->sigma * mean_sq()) * (1.0 + 8.0 * DBL_EPSILON) : h[0]);
    if (cn_in == nullptr) {
      cmax = h[1];
      csq = h[2];
      if (ic != nullptr) {
        amax = h[3];
        asq = h[4];
      }
    }
    if (grp != nullptr) {   // gcn[g] = ||A_[g]||_F / w_g and its maximum, which stands in for cmax
      launch_group_cnorm(cn, grp->ptr, grp->wts, grp->G, grp->max_run, w.gcn_full,
                         Red{w.part, w.ticket, w.red + 12}, st);
      check_launch();
      GLX_HIP(hipMemcpyAsync(&gcol_max, w.red + 12, sizeof(double), hipMemcpyDeviceToHost, st));
      GLX_HIP(hipStreamSynchronize(st));
    }
  }
  // the groups of the current (reduced) problem; gmap: its groups -> the full problem's (NULL: identity)
  GroupView gcur = grp != nullptr ? *grp : GroupView{};
  double sgl_extra[4] = {0.0, 0.0, 0.0, 0.0};   // [s, s of the padded solve, max rho, 0] of the last check
  if (sgl) {
    gcur.extra = sgl_extra;
    if (screen) {   // the padding of the second dual solve is the guard's, fixed for the whole solve
      double pad[2];
      sgl_guard_pad(dtype, m, l, grp->max_run, cmax, sw != nullptr, pad);
      gcur.pad_mul = pad[0];
      gcur.pad_add = pad[1];
    }
  }
  const double* gcn = w.gcn_full;
  const int* gmap = nullptr;
  int gside = 0;             // the description the next k_group_expand writes
  int64_t listed_g = 0;      // groups the last screen kept (valid with `listed`)

  // the current (reduced) problem
  const T* Ac = A;
  int64_t wc = n;
  FusePlan pl = fuse_plan(dtype, m, n, l);
  int side = 0;              // the buffer the next compaction writes
  const int* map = nullptr;  // reduced row -> full row (NULL: identity)
  int mapi = 0;
  T *x = static_cast<T*>(w.x[0]), *y = static_cast<T*>(w.x[1]), *xc = static_cast<T*>(w.x[2]),
    *yn = static_cast<T*>(w.x[3]), *vn = static_cast<T*>(w.x[4]);
  GLX_HIP(hipMemcpyAsync(x, X, es * n * l, hipMemcpyDeviceToDevice, st));
  GLX_HIP(hipMemcpyAsync(y, X, es * n * l, hipMemcpyDeviceToDevice, st));
  info->fused = pl.fuse_ok && grp == nullptr ? 1 : 0;

  double target = tol;
  int64_t k = 1;       // momentum index: theta = 2 / (k + 1)
  int64_t it = 0;
  bool all_zero = false;
  int64_t listed = -1;   // >= 0: entries of w.list from the last screen, valid for the current problem
  double rec[8];

  // x (reduced) -> X (n x l); then the certificate of the full problem on the caller's A. Where the
  // last check screened without compacting, only the rows it listed travel: a row proven zero is
  // returned as +0 whether a compaction dropped it or not (xc and the idle map are free here)
  auto full_certificate = [&]() {
    if (all_zero) {
      GLX_HIP(hipMemsetAsync(X, 0, es * n * l, st));
    } else if (listed >= 0) {   // (<= pad64(wc) entries, -1 behind the kept rows; none: X = 0)
      int* rows = w.map[mapi ^ 1];
      GLX_HIP(hipMemsetAsync(X, 0, es * n * l, st));
      launch_gather_rows<T>(x, w.list, listed, l, xc, st);
      launch_compose_list(map, w.list, listed, rows, st);
      launch_scatter_rows<T>(xc, rows, listed, l, X, st);
      check_launch();
    } else if (map == nullptr) {
      GLX_HIP(hipMemcpyAsync(X, x, es * n * l, hipMemcpyDeviceToDevice, st));
    } else {
      GLX_HIP(hipMemsetAsync(X, 0, es * n * l, st));
      launch_scatter_rows<T>(x, map, wc, l, X, st);
      check_launch();
    }
    cert_call(dtype, m, n, l, A, X, b, mu, nullptr, info->cert, w, st, grp, sw != nullptr ? &sw_out : nullptr,
              holdout_sum, ic);
    info->passes += 2.0;
    return compose(info->cert, mu);
  };

  // one check of the reduced problem: its certificate, the stop rule, the guard, the screen and,
  // where it pays, a compaction. Returns true when the reduced problem meets `target`.
  auto check = [&]() -> bool {
    ++info->checks;
    cert_call(dtype, m, wc, l, Ac, x, b, mu, w.rn, rec, w, st, grp != nullptr ? &gcur : nullptr,
              sw != nullptr ? &sw_in : nullptr, nullptr, ic);
    info->passes += 2.0 * (double)wc / (double)n;
    const Composed c = compose(rec, mu);
    info->inner_rel_gap = c.rel;
    const bool met = c.rel <= target;
    if (!screen) return met;
    double gd[4] = {0.0, 0.0, 0.0, 0.0};
    const double cst[4] = {cmax, csq, amax, asq};
    if (ic != nullptr && grp != nullptr)
      group_screen_guard_ic(rec, mu, dtype, m, wc, l, grp->max_run, grp->w_min, gcol_max, cst, bn, ic->sigma, mean_sq(),
                            gd);
    else if (ic != nullptr)
      screen_guard_ic(rec, mu, dtype, m, wc, l, cst, bn, ic->sigma, mean_sq(), gd);
    // the test's own three roundings in fp64 (intercept: and the guard's slack, gd[3], off mu)
    const double mu_lo = (mu - gd[3]) * (1.0 - 4.0 * DBL_EPSILON);
    int hc[4] = {0, 0, 0, 0};
    if (sgl) {   // the two-level test on the rows and the groups, then the rows that stay
      double g5[5];
      sgl_screen_guard(rec, sgl_extra[1], mu, tau, dtype, m, wc, l, grp->max_run, grp->w_min, cmax, csq, bn, g5,
                       sw != nullptr);
      const double shave = 1.0 - 8.0 * DBL_EPSILON;   // the tests' own roundings in fp64
      launch_sgl_screen(w.rn, cn, gcn, gcur.ptr, gcur.wts, gcur.G, g5[2], g5[0], g5[1], nullptr, g5[4],
                        tau * mu * shave, (1.0 - tau) * mu * shave, tau < 1.0 ? 1 : 0, w.skeep, nullptr,
                        Red{w.part, w.ticket, w.red + 14}, st);
      launch_sgl_expand(w.skeep, gcur.ptr, gcur.wts, gcn, gmap, gcur.G, w.list, w.gptr[gside], w.gw[gside],
                        w.ggcn[gside], w.gmap[gside], w.cnt, st);
      check_launch();
      GLX_HIP(hipMemcpyAsync(hc, w.cnt, sizeof hc, hipMemcpyDeviceToHost, st));
    } else if (grp != nullptr) {   // the same test on the G "rows" of groups, then their rows
      if (ic == nullptr)
        group_screen_guard(rec, mu, dtype, m, wc, l, grp->max_run, grp->w_min, gcol_max, csq, bn, gd, sw != nullptr);
      launch_screen(w.rn, gcn, gcur.G, gd[0], gd[2], mu_lo, nullptr, w.glist, w.cnt, w.bal, w.sticket, st);
      launch_group_expand(w.glist, w.cnt, gcur.ptr, gcur.wts, gcn, gmap, w.list, w.gptr[gside], w.gw[gside],
                          w.ggcn[gside], w.gmap[gside], w.cnt + 2, st);
      check_launch();
      GLX_HIP(hipMemcpyAsync(hc, w.cnt, sizeof hc, hipMemcpyDeviceToHost, st));
    } else {
      if (ic == nullptr) screen_guard(rec, mu, dtype, m, wc, l, cmax, csq, bn, gd, sw != nullptr);
      launch_screen(w.rn, cn, wc, gd[0], gd[2], mu_lo, nullptr, w.list, w.cnt, w.bal, w.sticket, st);
      check_launch();
      GLX_HIP(hipMemcpyAsync(hc, w.cnt, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    GLX_HIP(hipStreamSynchronize(st));
    const int64_t kept = hc[0], wp = grp != nullptr ? hc[3] : hc[1];   // (kept counts groups there)
    info->kept = kept;
    listed = wp;   // w.list names the rows of the current problem that are not proven zero
    listed_g = kept;
    if (met || wp * 10 > wc * 9) return met;
    if (kept == 0) {   // every row is zero at the optimum
      all_zero = true;
      wc = 0;
      listed = -1;
      if (info->compactions < GLX_CERTIFIED_MAX_HIST) info->kept_hist[info->compactions] = 0;
      if (sgl && grp->row_hist != nullptr && info->compactions < GLX_CERTIFIED_MAX_HIST)
        grp->row_hist[info->compactions] = 0;
      ++info->compactions;
      return true;
    }
    if (wp > w.cap[side]) throw Error{GLX_E_STATE, "certified solve: a compaction exceeds its buffer"};
    T* An = static_cast<T*>(w.abuf[side]);
    launch_gather_cols<T>(Ac, m, wc, w.list, wp, An, st);
    launch_gather_rows<T>(x, w.list, wp, l, xc, st);
    double* cnn = w.cn[cn == w.cn[0] ? 1 : 0];
    if (grp == nullptr || sgl) launch_gather_rows<double>(cn, w.list, wp, 1, cnn, st);
    int* mapn = w.map[mapi ^ 1];
    launch_compose_list(map, w.list, wp, mapn, st);
    check_launch();
    info->passes += (double)wc / (double)n;
    std::swap(x, xc);
    GLX_HIP(hipMemcpyAsync(y, x, es * wp * l, hipMemcpyDeviceToDevice, st));   // the momentum restarts
    k = 1;
    Ac = An;
    if (grp == nullptr || sgl) cn = cnn;
    if (grp != nullptr) {   // k_group_expand wrote the reduced description beside the row list
      gcur.ptr = w.gptr[gside];
      gcur.wts = w.gw[gside];
      gcur.G = kept;
      gcn = w.ggcn[gside];
      gmap = w.gmap[gside];
      gside ^= 1;
    }
    map = mapn;
    mapi ^= 1;
    side ^= 1;
    wc = wp;
    pl = fuse_plan(dtype, m, wc, l);
    if (info->compactions < GLX_CERTIFIED_MAX_HIST) info->kept_hist[info->compactions] = kept;
    if (sgl && grp->row_hist != nullptr && info->compactions < GLX_CERTIFIED_MAX_HIST)
      grp->row_hist[info->compactions] = hc[1];
    ++info->compactions;
    listed = -1;   // the composed list alone names them now
    return false;
  };

  auto iterate = [&]() {
    const double theta = 2.0 / (double)(k + 1), theta_next = 2.0 / (double)(k + 2);
    const T* xs[3] = {y, nullptr, nullptr};
    T* r = static_cast<T*>(w.r);
    launch_ax<T>(pl.a, 1, Ac, xs, static_cast<T*>(w.pa), nullptr, 0, st);
    if (ic != nullptr) {   // r = w (A y - b - 1 mean^T): the two centring launches, no readback
      launch_cert_csum<T>(static_cast<T*>(w.pa), ax_split(pl.a, 1), b, sww, static_cast<T*>(ic->rhat), m, l, ic->sigma,
                          ic->part, ic->cnt, ic->mean, st);
      launch_cert_fin_c<T>(static_cast<const T*>(ic->rhat), b, sww, nullptr, ic->mean, nullptr, r, ml, l, red0, st);
    } else if (sww != nullptr)   // r = w (A y - b): every step below takes it as the R it already takes
      launch_cert_fin_w<T>(static_cast<T*>(w.pa), ax_split(pl.a, 1), b, sww, nullptr, nullptr, r, ml, l, red0, st);
    else
      launch_cert_fin<T>(static_cast<T*>(w.pa), ax_split(pl.a, 1), b, r, ml, red0, st);
    T* gp = static_cast<T*>(w.gp);
    if (sgl) {   // the sparse-group step: A^T r, then the two-level prox on its slabs
      launch_atr<T>(pl.a, Ac, r, gp, st);
      launch_sgl_fista<T>(y, gp, pl.a.atr_S, x, xc, vn, yn, gcur.ptr, gcur.wts, gcur.G, wc, l, t, mu, tau, thres, theta,
                          theta_next, red1, st);
    } else if (grp != nullptr) {   // the grouped step is never fused: A^T r, then the group kernel on its slabs
      launch_atr<T>(pl.a, Ac, r, gp, st);
      launch_group_fista<T>(y, gp, pl.a.atr_S, x, xc, vn, yn, gcur.ptr, gcur.wts, gcur.G, wc, l, grp->max_run, t, mu,
                            thres, theta, theta_next, red1, st);
    } else if (pl.fuse_ok) {
      launch_atr_fista<T>(pl.a, Ac, r, static_cast<T*>(w.g), y, x, xc, vn, yn, t, mu, thres, theta, theta_next, red1,
                          st, Pub{}, pl.a.atr_S > 1 ? gp : nullptr, w.pcnt);
    } else {
      launch_atr<T>(pl.a, Ac, r, gp, st);
      launch_fista_trial<T>(true, y, gp, pl.a.atr_S, nullptr, x, xc, vn, yn, wc, l, t, mu, thres, theta, theta_next,
                            0.0, red1, st);
    }
    check_launch();
    std::swap(x, xc);
    std::swap(y, yn);
    ++k;
    ++it;
    info->passes += 2.0 * (double)wc / (double)n;
  };

  info->kept = grp != nullptr ? grp->G : n;
  Composed full{};
  for (int round = 0;; ++round) {
    info->rounds = round + 1;
    bool met = check();   // (the first: x0 may already do, and a warm start screens before it iterates)
    while (!met && !all_zero && it < maxit) {
      iterate();
      if (it % check_every == 0 || it >= maxit) met = check();
    }
    full = full_certificate();
    if (full.rel <= tol) {
      info->converged = 1;
      break;
    }
    if (it >= maxit || round + 1 >= 6 || all_zero) break;   // the first round and at most 5 resumed ones
    target *= 0.5;
  }
  // the rows not proven zero: the last screen's list through the composed one, or the latter alone
  if (kept_rows != nullptr && wc > 0 && listed > 0) {
    launch_compose_list(map, w.list, listed, kept_rows, st);
    check_launch();
    info->listed = listed;
  } else if (kept_rows != nullptr && wc > 0 && listed < 0 && map != nullptr) {
    GLX_HIP(hipMemcpyAsync(kept_rows, map, sizeof(int) * wc, hipMemcpyDeviceToDevice, st));
    info->listed = wc;
  }
  if (listed_groups != nullptr) *listed_groups = 0;
  if (grp != nullptr && kept_groups != nullptr && wc > 0 && (listed > 0 || gmap != nullptr)) {
    const int* src = listed > 0 ? w.gmap[gside] : gmap;   // the last expand's map, or the current problem's
    const int64_t cnt = listed > 0 ? listed_g : gcur.G;
    GLX_HIP(hipMemcpyAsync(kept_groups, src, sizeof(int) * cnt, hipMemcpyDeviceToDevice, st));
    if (listed_groups != nullptr) *listed_groups = cnt;
  }
  GLX_HIP(hipStreamSynchronize(st));
  info->iters = it;
  info->width = wc;
  info->tt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
}

// the one-launch entries' workspace: [partials | ticket | out | column partials | column counters |
// ballot words | screen ticket]
struct StepWs {
  double* part; unsigned* ticket; double* out; double* cpart; unsigned* ccnt; unsigned long long* bal;
  unsigned* sticket;
};
size_t step_carve(int64_t m, int64_t n, void* base, StepWs* out) {
  Carver c(base);
  StepWs w;
  w.part = static_cast<double*>(c.take(sizeof(double) * kMaxRedVals * kMaxBlocks));
  w.ticket = static_cast<unsigned*>(c.take(kTicketBytes));
  w.out = static_cast<double*>(c.take(sizeof(double) * kMaxRedVals));
  w.cpart = static_cast<double*>(c.take(col_norms_part_bytes(m, n)));
  w.ccnt = static_cast<unsigned*>(c.take(col_norms_count_bytes(n)));
  w.bal = static_cast<unsigned long long*>(c.take(screen_words_bytes(n)));
  w.sticket = static_cast<unsigned*>(c.take(256));
  if (out) *out = w;
  return c.off + 256;
}

}  // namespace

// The guard of the problem with an intercept (DESIGN.md "Intercept", "The guard, term by term"): the
// weighted guard on the centred record with
//   - the uncentred figures, which the roundings of A y and of A^T (w r_c) still see, recovered by
//     Pythagoras from the centred ones and the column means: max ||a~_i||^2 <= cmax^2 + sigma amax^2,
//     ||A~||_F^2 = csq + sigma asq, ||r~^||^2 = rec[0] + sigma mean_sq (py covers their own roundings);
//   - eps >= ||1~^T r~_c|| / sqrt(sigma), the departure of theta from the dual's equality: projecting
//     theta onto it moves it by s eps, costs the dual value s eps ||b~|| + 1/2 s^2 eps^2, adds s eps to
//     the radius and |a-bar_i| sqrt(sigma) s eps to a row's ||a~_i^T theta||;
//   - one more rounding of the residual (r_c in A's dtype) in dr;
//   - out[3], the slack: the terms that scale with the UNcentred norm of a column cannot ride on its
//     centred norm in  s rn + cn rho < mu  and are taken off mu instead.
void screen_guard_ic(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l, const double* cs,
                     double bn_in, double sigma, double mean_sq, double* out) {
  const double k = 3.0;
  const double u = dtype == GLX_F64 ? DBL_EPSILON : (double)FLT_EPSILON;
  const double u64 = DBL_EPSILON;
  const double rr = rec[0], rb = rec[1], sx = rec[2], gmax = rec[3];
  const double rn = std::sqrt(rr);
  const double gm = gamma_k((double)m + k, u), gn = gamma_k((double)n + 2.0, u);
  const double ml = (double)m * (double)l;
  const double g_ml = gamma_k(ml + k, u64);
  const double bn = bn_in * (1.0 + g_ml);
  const double up = 1.0 + gamma_k((double)m + 5.0, u64);   // the centred norms are low by at most this
  const double py = 1.0 + 3.0 * gamma_k((double)m + (double)n + 8.0, u64);
  const double cmax = cs[0], csq = cs[1], amax = cs[2], asq = cs[3];
  const double cu = std::sqrt((cmax * cmax * up * up + sigma * amax * amax) * py);
  const double csq_u = (csq + sigma * asq) * py;
  const double rhn = std::sqrt((rr + sigma * mean_sq) * py * (1.0 + 4.0 * u));
  const double eps = gamma_k(2.0, u) * rn + gamma_k((double)m + 3.0, u64) * rhn;
  const double dep = amax * std::sqrt(sigma) * eps * (1.0 + 4.0 * u64);
  // 1. dual feasibility of the projected point
  const double den = gmax + gm * cu * rn + dep;
  const double s = den > mu ? mu / den : (den <= mu ? 1.0 : den);   // (NaN den: NaN)
  // 2. the primal value, for the intercept the record's means give (any other only raises it)
  const double dr = gn * std::sqrt(csq_u) * sx + u * (rhn + 2.0 * bn) + u * rn;
  const double bar_rr = g_ml * rr;
  const double bar_rb = g_ml * rn * bn;
  const double bar_sx = (gamma_k((double)l + 2.0, u) + gamma_k((double)n + 2.0, u64)) * sx;
  const double gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * sx;
  const double bars = rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx +
                      s * eps * bn + 0.5 * s * s * eps * eps;
  const double gap_p = (gap > 0.0 ? gap : (gap <= 0.0 ? 0.0 : gap)) + bars;
  // 3. the radius on the centred norms, and the slack
  const double gl = gamma_k((double)l + 2.0, u);
  out[0] = s;
  out[1] = gap_p;
  out[2] = (std::sqrt(2.0 * gap_p) + s * eps) * up;
  out[3] = s * (gm * cu * rn + gl * (1.0 + gm) * cu * rn + dep) * (1.0 + 8.0 * u64);
}

size_t certified_bytes(int dtype, int64_t m, int64_t n, int64_t l, bool screen, int64_t G, bool weighted,
                       bool intercept, bool sgl) {
  check_shape(dtype, m, n, l);
  return carve(dtype, m, n, l, screen, true, nullptr, nullptr, G, weighted, intercept, sgl);
}

std::string certified_describe(int dtype, int64_t m, int64_t n, int64_t l, bool screen, int64_t max_run, bool sgl) {
  check_shape(dtype, m, n, l);
  return describe_certified(dtype, m, n, l, screen, max_run, sgl);
}

void certified_run(const glx_problem* prob, double t, double tol, int64_t maxit, int screen, int check_every,
                   const double* col_norms_dev, const double* col_stats, int32_t* kept_rows_dev, void* ws,
                   size_t wsb, glx_certified_info* info, void* stream, const GroupView* grp,
                   int32_t* kept_groups_dev, int64_t* listed_groups, const SampleView* sw, double* holdout_sum,
                   const InterceptView* ic) {
  if (!prob || !info) throw Error{GLX_E_INVALID, "null problem/info"};
  if (ic != nullptr) check_intercept(ic->sigma, ic->mean_host);
  if (grp != nullptr && !(grp->row_ratio >= 0.0 && grp->row_ratio <= 1.0))
    throw Error{GLX_E_INVALID, "row_ratio must be in [0, 1] (and not NaN)"};
  if (grp != nullptr && grp->row_ratio > 0.0 && ic != nullptr)
    throw Error{GLX_E_INVALID, "the sparse-group penalty (row_ratio > 0) takes no intercept"};
  if (sw != nullptr) check_sample(sw->w, sw->hold);
  if (sw != nullptr && sw->w == nullptr) throw Error{GLX_E_INVALID, "sample weights: null vector"};
  if (prob->comm != nullptr) throw Error{GLX_E_INVALID, "the certified solve is single-GPU: comm must be NULL"};
  check_shape(prob->dtype, prob->m, prob->n, prob->l);
  if (!(prob->mu0 >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
  if (!(t > 0.0) || !std::isfinite(t)) throw Error{GLX_E_INVALID, "the step t must be positive and finite"};
  if (!(tol > 0.0)) throw Error{GLX_E_INVALID, "tol must be positive"};
  if (maxit < 0) throw Error{GLX_E_INVALID, "negative iteration limit"};
  if (check_every < 1) throw Error{GLX_E_INVALID, "check_every must be >= 1"};
  if (!prob->A || !prob->b || !prob->x) throw Error{GLX_E_INVALID, "A, b and x must be device pointers"};
  if ((reinterpret_cast<uintptr_t>(prob->A) | reinterpret_cast<uintptr_t>(prob->b) |
       reinterpret_cast<uintptr_t>(prob->x)) & 15)
    throw Error{GLX_E_INVALID, "A, b, x must be 16-byte aligned"};
  if ((col_norms_dev != nullptr) != (col_stats != nullptr))
    throw Error{GLX_E_INVALID, "col_norms_dev and col_stats go together"};
  check_workspace(carve(prob->dtype, prob->m, prob->n, prob->l, screen != 0, true, nullptr, nullptr,
                        grp != nullptr ? grp->G : 0, sw != nullptr || ic != nullptr, ic != nullptr,
                        grp != nullptr && grp->row_ratio > 0.0),
                  ws, wsb, GLX_E_INVALID,
                  grp != nullptr ? "glx_group_certified_workspace_bytes" : "glx_certified_workspace_bytes");
  if (holdout_sum != nullptr) *holdout_sum = 0.0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  by_dtype(prob->dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    solve<T>(prob->dtype, prob->m, prob->n, prob->l, (const T*)prob->A, (const T*)prob->b, (T*)prob->x, prob->mu0, t,
             tol, maxit, screen != 0, check_every, col_norms_dev, col_stats, kept_rows_dev, ws, info, st, grp,
             kept_groups_dev, listed_groups, sw, holdout_sum, ic);
  });
}

}  // namespace glx

using namespace glx;

extern "C" {

int glx_screen_guard(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l, double col_max,
                     double col_sumsq, double b_norm, double* out) {
  return guarded([&] {
    if (!rec || !out) throw Error{GLX_E_INVALID, "null argument"};
    check_shape(dtype, m, n, l);
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    screen_guard(rec, mu, dtype, m, n, l, col_max, col_sumsq, b_norm, out);
  });
}

int glx_screen_workspace_bytes(int64_t m, int64_t n, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (m <= 0 || n <= 0) throw Error{GLX_E_INVALID, "m, n must be positive"};
    *bytes = step_carve(m, n, nullptr, nullptr);
  });
}

int glx_col_norms(int dtype, int64_t m, int64_t n, const void* A, double* norms_dev, double* stats_dev, void* ws,
                  size_t wsb, void* stream) {
  return guarded([&] {
    check_shape(dtype, m, n, 1);
    if (!A || !norms_dev || !stats_dev) throw Error{GLX_E_INVALID, "null argument"};
    check_workspace(step_carve(m, n, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_screen_workspace_bytes");
    StepWs w;
    step_carve(m, n, ws, &w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    GLX_HIP(hipMemsetAsync(w.ccnt, 0, col_norms_count_bytes(n), st));
    const Red red{w.part, w.ticket, stats_dev};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_col_norms<T>((const T*)A, m, n, norms_dev, w.cpart, w.ccnt, red, st);
    });
    check_launch();
  });
}

int glx_screen_step(int64_t n, const double* row_norms, const double* col_norms, double s, double rho, double mu,
                    uint8_t* mask, int32_t* list, int32_t* count, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    if (n <= 0 || n > (int64_t)0x7fffffc0) throw Error{GLX_E_INVALID, "n must be in 1 .. 2^31 - 65"};
    if (!row_norms || !col_norms || !list || !count) throw Error{GLX_E_INVALID, "null argument"};
    check_workspace(step_carve(1, n, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_screen_workspace_bytes");
    StepWs w;
    step_carve(1, n, ws, &w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLX_HIP(hipMemsetAsync(w.sticket, 0, 256, st));
    launch_screen(row_norms, col_norms, n, s, rho, mu, mask, list, count, w.bal, w.sticket, st);
    check_launch();
  });
}

int glx_gather_cols(int dtype, int64_t m, int64_t src_width, const void* src, const int32_t* idx, int64_t width,
                    void* dst, void* stream) {
  return guarded([&] {
    check_dtype(dtype);
    if (m <= 0 || src_width <= 0 || width < 0) throw Error{GLX_E_INVALID, "bad shape"};
    if (width % 64 != 0) throw Error{GLX_E_INVALID, "the destination width must be a multiple of 64"};
    if (width == 0) return;
    if (!src || !idx || !dst) throw Error{GLX_E_INVALID, "null argument"};
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_gather_cols<T>((const T*)src, m, src_width, idx, width, (T*)dst, st);
    });
    check_launch();
  });
}

int glx_certified_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int screen, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    check_shape(dtype, m, n, l);
    *bytes = carve(dtype, m, n, l, screen != 0, true, nullptr, nullptr);
  });
}

int glx_certified_describe(int dtype, int64_t m, int64_t n, int64_t l, int screen, char* out, size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    check_shape(dtype, m, n, l);
    std::snprintf(out, cap, "%s", describe_certified(dtype, m, n, l, screen != 0).c_str());
  });
}

int glx_certified_solve(const glx_problem* prob, double t, double tol, int64_t maxit, int screen, int check_every,
                        const double* col_norms_dev, const double* col_stats, int32_t* kept_rows_dev,
                        void* ws, size_t wsb, glx_certified_info* info, void* stream) {
  return guarded([&] {
    certified_run(prob, t, tol, maxit, screen, check_every, col_norms_dev, col_stats, kept_rows_dev, ws, wsb, info,
                  stream, nullptr, nullptr, nullptr);
  });
}

/* ---- sample weights (DESIGN.md "Sample weights and cross-validation") ---- */

int glx_screen_guard_sw(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l, double col_max,
                        double col_sumsq, double b_norm, double* out) {
  return guarded([&] {
    if (!rec || !out) throw Error{GLX_E_INVALID, "null argument"};
    check_shape(dtype, m, n, l);
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    screen_guard(rec, mu, dtype, m, n, l, col_max, col_sumsq, b_norm, out, true);
  });
}

int glx_col_norms_sw(int dtype, int64_t m, int64_t n, const void* A, const void* sample_w, double* norms_dev,
                     double* stats_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_shape(dtype, m, n, 1);
    if (!A || !sample_w || !norms_dev || !stats_dev) throw Error{GLX_E_INVALID, "null argument"};
    check_sample(sample_w, nullptr);
    check_workspace(step_carve(m, n, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_screen_workspace_bytes");
    StepWs w;
    step_carve(m, n, ws, &w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    GLX_HIP(hipMemsetAsync(w.ccnt, 0, col_norms_count_bytes(n), st));
    const Red red{w.part, w.ticket, stats_dev};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_col_norms_w<T>((const T*)A, (const T*)sample_w, m, n, norms_dev, w.cpart, w.ccnt, red, st);
    });
    check_launch();
  });
}

int glx_cert_fin_sw(int dtype, int64_t m, int64_t l, const void* P, int S, const void* b, const void* sample_w,
                    const void* holdout_w, void* r_out, void* rw_out, double* sums_dev, void* ws, size_t wsb,
                    void* stream) {
  return guarded([&] {
    check_shape(dtype, m, 1, l);
    if (S < 0 || S > kMaxSplit) throw Error{GLX_E_INVALID, "S must be in 0 .. 64"};
    if ((S > 0) != (P != nullptr)) throw Error{GLX_E_INVALID, "P goes with S > 0"};
    if (!b || !rw_out || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    check_sample(sample_w, holdout_w);
    check_workspace(step_carve(1, 1, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_screen_workspace_bytes");
    StepWs w;
    step_carve(1, 1, ws, &w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    const Red red{w.part, w.ticket, sums_dev};
    const int64_t ml = m * l;
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      if (sample_w != nullptr)
        launch_cert_fin_w<T>((const T*)P, S, (const T*)b, (const T*)sample_w, (const T*)holdout_w, (T*)r_out,
                             (T*)rw_out, ml, l, red, st);
      else   // the unweighted finalize, for the bit comparison: rw_out = r, two sums
        launch_cert_fin<T>((const T*)P, S, (const T*)b, (T*)rw_out, ml, red, st);
    });
    check_launch();
  });
}

int glx_certified_sw_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int screen, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    check_shape(dtype, m, n, l);
    *bytes = carve(dtype, m, n, l, screen != 0, true, nullptr, nullptr, 0, true);
  });
}

int glx_certified_sw_describe(int dtype, int64_t m, int64_t n, int64_t l, int screen, char* out, size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    check_shape(dtype, m, n, l);
    std::snprintf(out, cap, "%s; residual=weighted finalize (k_cert_fin_w)",
                  describe_certified(dtype, m, n, l, screen != 0).c_str());
  });
}

int glx_certified_solve_sw(const glx_problem* prob, const void* sample_w, const void* holdout_w, double t, double tol,
                           int64_t maxit, int screen, int check_every, const double* col_norms_dev,
                           const double* col_stats, int32_t* kept_rows_dev, void* ws, size_t wsb,
                           glx_certified_info* info, double* holdout_sum, void* stream) {
  return guarded([&] {
    check_sample(sample_w, holdout_w);
    if (holdout_sum != nullptr) *holdout_sum = 0.0;
    if (sample_w == nullptr) {   // today's entry, call for call (its workspace is a prefix of this one's)
      certified_run(prob, t, tol, maxit, screen, check_every, col_norms_dev, col_stats, kept_rows_dev, ws, wsb, info,
                    stream, nullptr, nullptr, nullptr);
      return;
    }
    const SampleView sw{sample_w, holdout_w, nullptr};
    certified_run(prob, t, tol, maxit, screen, check_every, col_norms_dev, col_stats, kept_rows_dev, ws, wsb, info,
                  stream, nullptr, nullptr, nullptr, &sw, holdout_sum);
  });
}

/* ---- the unpenalised intercept (DESIGN.md "Intercept") ---- */

int glx_screen_guard_ic(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l,
                        const double* col_stats, double b_norm, double weight_sum, double mean_sq, double* out) {
  return guarded([&] {
    if (!rec || !out || !col_stats) throw Error{GLX_E_INVALID, "null argument"};
    check_shape(dtype, m, n, l);
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    if (!(weight_sum > 0.0) || !std::isfinite(weight_sum))
      throw Error{GLX_E_INVALID, "intercept: weight_sum must be positive and finite"};
    screen_guard_ic(rec, mu, dtype, m, n, l, col_stats, b_norm, weight_sum, mean_sq, out);
  });
}

namespace {
// the one-launch intercept entries' workspace: [glx_screen_workspace_bytes(m, n) | column means |
// the centring finalize's partials | its counter]
struct IcStepWs {
  double* cmean;
  double* part;
  unsigned* cnt;
};
size_t ic_step_carve(int64_t m, int64_t n, void* base, StepWs* head, IcStepWs* out) {
  Carver c(base);
  c.take(step_carve(m, n, base, head) - 256);
  IcStepWs w;
  w.cmean = static_cast<double*>(c.take(sizeof(double) * (size_t)n));
  w.part = static_cast<double*>(c.take(cert_csum_part_bytes()));
  w.cnt = static_cast<unsigned*>(c.take(256));
  if (out) *out = w;
  return c.off + 256;
}
}  // namespace

int glx_intercept_workspace_bytes(int64_t m, int64_t n, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (m <= 0 || n <= 0) throw Error{GLX_E_INVALID, "m, n must be positive"};
    *bytes = ic_step_carve(m, n, nullptr, nullptr, nullptr);
  });
}

int glx_col_norms_ic(int dtype, int64_t m, int64_t n, const void* A, const void* sample_w, double weight_sum,
                     double* norms_dev, double* means_dev, double* stats_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_shape(dtype, m, n, 1);
    if (!A || !norms_dev || !means_dev || !stats_dev) throw Error{GLX_E_INVALID, "null argument"};
    check_sample(sample_w, nullptr);
    if (!(weight_sum > 0.0) || !std::isfinite(weight_sum))
      throw Error{GLX_E_INVALID, "intercept: weight_sum must be positive and finite"};
    check_workspace(ic_step_carve(m, n, nullptr, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                    "glx_intercept_workspace_bytes");
    StepWs w;
    ic_step_carve(m, n, ws, &w, nullptr);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    GLX_HIP(hipMemsetAsync(w.ccnt, 0, col_norms_count_bytes(n), st));
    const Red red{w.part, w.ticket, stats_dev}, red_mean{w.part, w.ticket, stats_dev + 2};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_col_norms_c<T>((const T*)A, (const T*)sample_w, weight_sum, m, n, norms_dev, means_dev, w.cpart, w.ccnt,
                            red_mean, red, st);
    });
    check_launch();
  });
}

int glx_cert_fin_ic(int dtype, int64_t m, int64_t l, const void* P, int S, const void* b, const void* sample_w,
                    const void* holdout_w, double weight_sum, void* rhat_out, double* means_dev, void* rc_out,
                    void* rw_out, double* sums_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_shape(dtype, m, 1, l);
    if (S < 0 || S > kMaxSplit) throw Error{GLX_E_INVALID, "S must be in 0 .. 64"};
    if ((S > 0) != (P != nullptr)) throw Error{GLX_E_INVALID, "P goes with S > 0"};
    if (!b || !rhat_out || !means_dev || !rw_out || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    if ((reinterpret_cast<uintptr_t>(sample_w) | reinterpret_cast<uintptr_t>(holdout_w)) & 15)
      throw Error{GLX_E_INVALID, "sample_w and holdout_w must be 16-byte aligned"};
    if (!(weight_sum > 0.0) || !std::isfinite(weight_sum))
      throw Error{GLX_E_INVALID, "intercept: weight_sum must be positive and finite"};
    check_workspace(ic_step_carve(1, 1, nullptr, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                    "glx_intercept_workspace_bytes");
    StepWs w;
    IcStepWs iw;
    ic_step_carve(1, 1, ws, &w, &iw);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    GLX_HIP(hipMemsetAsync(iw.cnt, 0, 256, st));
    const Red red{w.part, w.ticket, sums_dev};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_cert_csum<T>((const T*)P, S, (const T*)b, (const T*)sample_w, (T*)rhat_out, m, l, weight_sum, iw.part,
                          iw.cnt, means_dev, st);
      launch_cert_fin_c<T>((const T*)rhat_out, (const T*)b, (const T*)sample_w, (const T*)holdout_w, means_dev,
                           (T*)rc_out, (T*)rw_out, m * l, l, red, st);
    });
    check_launch();
  });
}

int glx_certified_ic_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int screen, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    check_shape(dtype, m, n, l);
    *bytes = carve(dtype, m, n, l, screen != 0, true, nullptr, nullptr, 0, true, true);
  });
}

int glx_certified_ic_describe(int dtype, int64_t m, int64_t n, int64_t l, int screen, char* out, size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    check_shape(dtype, m, n, l);
    std::snprintf(out, cap, "%s; residual=centring finalize (k_cert_csum, k_cert_fin_c)",
                  describe_certified(dtype, m, n, l, screen != 0).c_str());
  });
}

int glx_certified_solve_ic(const glx_problem* prob, const void* sample_w, const void* holdout_w, double weight_sum,
                           double t, double tol, int64_t maxit, int screen, int check_every,
                           const double* col_norms_dev, const double* col_stats, int32_t* kept_rows_dev, void* ws,
                           size_t wsb, glx_certified_info* info, double* holdout_sum, double* intercept_out,
                           void* stream) {
  return guarded([&] {
    check_sample(sample_w, holdout_w);
    check_intercept(weight_sum, intercept_out);
    if (holdout_sum != nullptr) *holdout_sum = 0.0;
    const SampleView sw{sample_w, holdout_w, nullptr};
    InterceptView ic;
    ic.sigma = weight_sum;
    ic.mean_host = intercept_out;
    certified_run(prob, t, tol, maxit, screen, check_every, col_norms_dev, col_stats, kept_rows_dev, ws, wsb, info,
                  stream, nullptr, nullptr, nullptr, sample_w != nullptr ? &sw : nullptr, holdout_sum, &ic);
    for (int64_t c = 0; c < prob->l; ++c) intercept_out[c] = -intercept_out[c];   // c = -r-bar
  });
}

}  // extern "C"
