// group.cpp — feature groups and weights (DESIGN.md "Feature groups and weights"): the C entries of
//   P(x) = 1/2 ||A x - b||_F^2 + mu sum_g w_g ||x_[g]||_F,   [g] = rows ptr[g] .. ptr[g + 1] - 1 of x.
// The certificate and the certified solve are the row ones' (certificate.cpp certificate_run,
// screen.cpp certified_run) with a GroupView: this unit validates the caller's host description of
// the groups before any launch, uploads it behind the callee's workspace, composes the grouped
// rounding guard and exposes the four kernels of kernels_group.hip one launch at a time.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "glx_host.h"

namespace glx {
namespace {

// What the host knows of a valid description: the figures the layout and the guard need.
struct GroupFacts {
  int64_t max_run = 1;
  double w_min = 1.0;
};
// GLX_E_INVALID for a description that is not G >= 1 strictly increasing offsets from 0 to n with
// positive finite weights (host arrays: nothing is launched before this passes).
GroupFacts check_groups(int64_t n, int64_t G, const int32_t* ptr, const double* wts) {
  if (G < 1) throw Error{GLX_E_INVALID, "groups: G must be >= 1"};
  if (!ptr || !wts) throw Error{GLX_E_INVALID, "groups: group_ptr and weights must be host arrays"};
  if (G > n) throw Error{GLX_E_INVALID, "groups: more groups than rows"};
  if (ptr[0] != 0) throw Error{GLX_E_INVALID, "groups: group_ptr[0] must be 0"};
  if ((int64_t)ptr[G] != n) throw Error{GLX_E_INVALID, "groups: group_ptr[G] must be n"};
  GroupFacts f;
  f.w_min = std::numeric_limits<double>::infinity();
  for (int64_t g = 0; g < G; ++g) {
    const int64_t run = (int64_t)ptr[g + 1] - (int64_t)ptr[g];
    if (run < 1) throw Error{GLX_E_INVALID, "groups: group_ptr must be strictly increasing"};
    if (!(wts[g] > 0.0) || !std::isfinite(wts[g]))
      throw Error{GLX_E_INVALID, "groups: every weight must be positive and finite"};
    f.max_run = std::max(f.max_run, run);
    f.w_min = std::min(f.w_min, wts[g]);
  }
  return f;
}
void check_dims(int dtype, int64_t n, int64_t l) {
  check_dtype(dtype);
  if (n <= 0 || l <= 0) throw Error{GLX_E_INVALID, "n, l must be positive"};
  if (l > kMaxL) throw Error{GLX_E_INVALID, "the group entries take l <= 128"};
  if (n > (int64_t)0x7fffffc0) throw Error{GLX_E_INVALID, "the group entries take n < 2^31 - 64"};
}
// the description's device copy, behind `head` bytes of the callee's workspace
struct GroupDev {
  void* head;
  int* ptr;
  double* wts;
};
size_t group_carve(size_t head, int64_t G, void* base, GroupDev* out) {
  Carver c(base);
  GroupDev d;
  d.head = c.take(head);
  d.ptr = static_cast<int*>(c.take(sizeof(int) * (size_t)(G + 1)));
  d.wts = static_cast<double*>(c.take(sizeof(double) * (size_t)G));
  if (out) *out = d;
  return c.off + 256;
}
// (the host arrays are the caller's and may go away after the call: the copies are complete on return).
// A float32 problem takes its weights rounded to float32 here, once, so that the step, the
// certificate and gcn all speak of the same problem.
GroupView upload(int dtype, const GroupDev& d, int64_t G, const int32_t* ptr, const double* wts,
                 const GroupFacts& f, hipStream_t st) {
  std::vector<double> wr;
  if (dtype == GLX_F32) {
    wr.resize((size_t)G);
    for (int64_t g = 0; g < G; ++g) {
      wr[(size_t)g] = (double)(float)wts[g];
      if (!(wr[(size_t)g] > 0.0) || !std::isfinite(wr[(size_t)g]))
        throw Error{GLX_E_INVALID, "groups: every weight must be positive and finite in float32"};
    }
    wts = wr.data();
  }
  GLX_HIP(hipMemcpyAsync(d.ptr, ptr, sizeof(int) * (size_t)(G + 1), hipMemcpyHostToDevice, st));
  GLX_HIP(hipMemcpyAsync(d.wts, wts, sizeof(double) * (size_t)G, hipMemcpyHostToDevice, st));
  GLX_HIP(hipStreamSynchronize(st));
  GroupView v;
  v.ptr = d.ptr;
  v.wts = d.wts;
  v.G = G;
  v.max_run = f.max_run;
  v.w_min = dtype == GLX_F32 ? (double)(float)f.w_min : f.w_min;
  return v;
}

size_t cert_bytes(int dtype, int64_t m, int64_t n, int64_t l) {
  size_t b = 0;
  if (glx_certificate_workspace_bytes(dtype, m, n, l, &b) != GLX_OK) throw Error{GLX_E_INVALID, g_last_error};
  return b;
}

// the one-launch entries' head: [partials | ticket]
constexpr size_t kStepHead = sizeof(double) * kMaxRedVals * kMaxBlocks + 256 + kTicketBytes;
struct StepWs {
  double* part;
  unsigned* ticket;
};
StepWs step_head(void* head) {
  Carver c(head);
  StepWs w;
  w.part = static_cast<double*>(c.take(sizeof(double) * kMaxRedVals * kMaxBlocks));
  w.ticket = static_cast<unsigned*>(c.take(kTicketBytes));
  return w;
}

}  // namespace

// The grouped rounding guard (DESIGN.md "Feature groups and weights", "The guard"). rec: the group
// certificate's record of the stored r^ and g^ = A^T r^ in dtype arithmetic. Every quantity is an
// upper bound; NaN propagates (and then keeps every group in k_screen).
void group_screen_guard(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run,
                        double w_min, double gcol_max, double csq, double bn_in, double* out, bool weighted) {
  // weighted (sample weights): one more rounding in w r^, in the two fp64 sums and in the column norms,
  // exactly as in screen_guard (DESIGN.md "Sample weights and cross-validation", "The guard")
  const double k = weighted ? 3.0 : 2.0;
  const double u = dtype == GLX_F64 ? DBL_EPSILON : (double)FLT_EPSILON;   // eps of A's dtype
  const double u64 = DBL_EPSILON;
  const double rr = rec[0], rb = rec[1], sxw = rec[2], gmax = rec[3];
  const double rn = std::sqrt(rr);
  const double K = (double)max_run * (double)l;   // terms of a group's norm
  const double gm = gamma_k((double)m + k, u), gn = gamma_k((double)n + 2.0, u);
  const double gK = gamma_k(K + 3.0, u);          // the norm in A's dtype, then the weight's rounding
  const double ml = (double)m * (double)l;
  const double g_ml = gamma_k(ml + k, u64);
  const double bn = weighted ? bn_in * (1.0 + g_ml) : bn_in;
  // the stored gcn are low by the column norms' gamma64_{m+2} and their own root and division
  const double up = (1.0 + gamma_k((double)m + k, u64)) * (1.0 + gamma_k((double)max_run + 3.0, u64));
  // 1. dual feasibility: ||A_[g]^T r^|| / w_g <= ||g^_[g]|| / w_g + gm (||A_[g]||_F / w_g) ||r^||, the
  //    per-column bounds summed in squares; the stored maximum may be low by its own gK
  const double den = gmax * (1.0 + gK) + gm * gcol_max * up * rn;
  const double s = den > mu ? mu / den : (den <= mu ? 1.0 : den);   // (NaN den: NaN)
  // 2. the primal value: ||x||_F <= sum_g ||x_[g]|| <= rec[2] / w_min
  const double dr = gn * std::sqrt(csq) * (sxw / w_min) + u * (rn + 2.0 * bn);
  const double bar_rr = g_ml * rr;
  const double bar_rb = g_ml * rn * bn;
  const double bar_sx = (gK + gamma_k((double)n + 2.0, u64)) * sxw;   // at most n groups in the fp64 sum
  const double gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * sxw;
  const double bars = rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx;
  const double gap_p = (gap > 0.0 ? gap : (gap <= 0.0 ? 0.0 : gap)) + bars;
  // 3. the group's own value: s ||A_[g]^T r^|| / w_g <= s rn[g] (1 + gK) + s gm (||A_[g]||_F / w_g) ||r^||
  //    and rn[g] <= (1 + gm) (||A_[g]||_F / w_g) ||r^||, so both are gcn[g] times a radius
  double rho = std::sqrt(2.0 * gap_p) + s * gm * rn + s * gK * (1.0 + gm) * rn;
  rho *= up;
  out[0] = s;
  out[1] = gap_p;
  out[2] = rho;
}

// The grouped guard of the problem with an intercept: screen_guard_ic's substitutions (screen.cpp; DESIGN.md
// "Intercept", "The guard") in group_screen_guard. A group's uncentred figure is at most
// sqrt(gcn_c^2 + sigma max_run amax^2 / w_min^2) and its share of the departure from 1~^T theta = 0 at
// most sqrt(max_run sigma) amax eps / w_min.
void group_screen_guard_ic(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run,
                           double w_min, double gcol_max, const double* cs, double bn_in, double sigma,
                           double mean_sq, double* out) {
  const double k = 3.0;
  const double u = dtype == GLX_F64 ? DBL_EPSILON : (double)FLT_EPSILON;
  const double u64 = DBL_EPSILON;
  const double rr = rec[0], rb = rec[1], sxw = rec[2], gmax = rec[3];
  const double rn = std::sqrt(rr);
  const double K = (double)max_run * (double)l;
  const double gm = gamma_k((double)m + k, u), gn = gamma_k((double)n + 2.0, u);
  const double gK = gamma_k(K + 3.0, u);
  const double ml = (double)m * (double)l;
  const double g_ml = gamma_k(ml + k, u64);
  const double bn = bn_in * (1.0 + g_ml);
  const double up = (1.0 + gamma_k((double)m + 5.0, u64)) * (1.0 + gamma_k((double)max_run + 3.0, u64));
  const double py = 1.0 + 3.0 * gamma_k((double)m + (double)n + 8.0, u64);
  const double csq = cs[1], amax = cs[2], asq = cs[3];
  const double ga = std::sqrt((double)max_run * sigma) * amax / w_min;   // a group's mean part / w_g
  const double gcu = std::sqrt((gcol_max * gcol_max * up * up + ga * ga) * py);
  const double csq_u = (csq + sigma * asq) * py;
  const double rhn = std::sqrt((rr + sigma * mean_sq) * py * (1.0 + 4.0 * u));
  const double eps = gamma_k(2.0, u) * rn + gamma_k((double)m + 3.0, u64) * rhn;
  const double dep = ga * eps * (1.0 + 4.0 * u64);
  const double den = gmax * (1.0 + gK) + gm * gcu * rn + dep;
  const double s = den > mu ? mu / den : (den <= mu ? 1.0 : den);
  const double dr = gn * std::sqrt(csq_u) * (sxw / w_min) + u * (rhn + 2.0 * bn) + u * rn;
  const double bar_rr = g_ml * rr;
  const double bar_rb = g_ml * rn * bn;
  const double bar_sx = (gK + gamma_k((double)n + 2.0, u64)) * sxw;
  const double gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * sxw;
  const double bars = rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx +
                      s * eps * bn + 0.5 * s * s * eps * eps;
  const double gap_p = (gap > 0.0 ? gap : (gap <= 0.0 ? 0.0 : gap)) + bars;
  out[0] = s;
  out[1] = gap_p;
  out[2] = (std::sqrt(2.0 * gap_p) + s * eps) * up;
  out[3] = s * (gm * gcu * rn + gK * (1.0 + gm) * gcu * rn + dep) * (1.0 + 8.0 * u64);
}

// The sparse-group guard (DESIGN.md "Sparse-group lasso", "The guard"). Feasibility is no single maximum
// here: the guard pads the row norms, p_i = mul rho^_i + add ||r^|| >= ||a_i^T r^|| for every row, and the
// dual-scale kernel's solve on the p_i gives an s that is feasible for the exact problem.
//   mul: ||g^_i|| <= rho^_i (1 + gl), the l-term norm in A's dtype; times ev, which covers phi's own
//        evaluation in fp64 (a sum of max_run squares, a root, a product and a difference per row) and the
//        roundings of a = tau mu and c_g = (1 - tau) mu w_g: phi(s; (1 + e) p) >= (1 + e) phi(s; p) for a >= 0
//   add: ||a_i^T r^ - g^_i|| <= gm ||a_i|| ||r^||, the per-column bounds summed in squares, with the stored
//        column norms low by gamma64_{m+k} and ||r^|| <= sqrt(rec[0]) (1 + g_ml); the device's root: 4 u64
void sgl_guard_pad(int dtype, int64_t m, int64_t l, int64_t max_run, double cmax, bool weighted, double* pad) {
  const double k = weighted ? 3.0 : 2.0;
  const double u = dtype == GLX_F64 ? DBL_EPSILON : (double)FLT_EPSILON;
  const double u64 = DBL_EPSILON;
  const double gm = gamma_k((double)m + k, u), gl = gamma_k((double)l + 2.0, u);
  const double ev = 1.0 + gamma_k((double)max_run + 16.0, u64);
  const double g_ml = gamma_k((double)m * (double)l + k, u64);
  pad[0] = (1.0 + gl) * ev;
  pad[1] = gm * cmax * (1.0 + gamma_k((double)m + k, u64)) * (1.0 + g_ml) * ev * (1.0 + 4.0 * u64);
}

// rec: the sparse-group record [||r^||^2, <r^, b>, Omega_tau(x), ...]; s_pad: min_g s_g of the padded
// solve. out = [mul, add ||r^||, s_safe, gap+, rho+]; group_screen_guard's items 2 and 3 with
//   - ||x||_F <= Omega_tau(x) / (tau + (1 - tau) w_min), both terms of Omega_tau bounding ||x||_F from above;
//   - Omega_tau's own error: a (max_run l)-term norm, the weight's and the ratio's products in A's dtype,
//     at most 2 n terms in the fp64 sum;
//   - the row's and the group's own values carried by the padding, so rho+ is the ball's radius lifted by
//     what the stored column and group norms may be low by.
// NaN propagates (and then keeps every row and group in k_sgl_screen).
void sgl_screen_guard(const double* rec, double s_pad, double mu, double tau, int dtype, int64_t m, int64_t n,
                      int64_t l, int64_t max_run, double w_min, double cmax, double csq, double bn_in, double* out,
                      bool weighted) {
  const double k = weighted ? 3.0 : 2.0;
  const double u = dtype == GLX_F64 ? DBL_EPSILON : (double)FLT_EPSILON;
  const double u64 = DBL_EPSILON;
  const double rr = rec[0], rb = rec[1], om = rec[2];
  const double rn = std::sqrt(rr);
  const double K = (double)max_run * (double)l;
  const double gn = gamma_k((double)n + 2.0, u);
  const double gK = gamma_k(K + 4.0, u);
  const double g_ml = gamma_k((double)m * (double)l + k, u64);
  const double bn = weighted ? bn_in * (1.0 + g_ml) : bn_in;
  const double up = (1.0 + gamma_k((double)m + k, u64)) * (1.0 + gamma_k((double)max_run + 3.0, u64));
  double pad[2];
  sgl_guard_pad(dtype, m, l, max_run, cmax, weighted, pad);
  const double s = s_pad < 1.0 ? s_pad : (s_pad >= 1.0 ? 1.0 : s_pad);   // (NaN: NaN)
  const double wq = tau + (1.0 - tau) * w_min;
  const double dr = gn * std::sqrt(csq) * (om / wq) + u * (rn + 2.0 * bn);
  const double bar_rr = g_ml * rr;
  const double bar_rb = g_ml * rn * bn;
  const double bar_sx = (gK + gamma_k(2.0 * (double)n + 2.0, u64)) * om;
  const double gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * om;
  const double bars = rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx;
  const double gap_p = (gap > 0.0 ? gap : (gap <= 0.0 ? 0.0 : gap)) + bars;
  out[0] = pad[0];
  out[1] = pad[1] * rn;
  out[2] = s;
  out[3] = gap_p;
  out[4] = std::sqrt(2.0 * gap_p) * up;
}

namespace {

void check_ratio(double tau) {
  if (!(tau >= 0.0 && tau <= 1.0)) throw Error{GLX_E_INVALID, "row_ratio must be in [0, 1] (and not NaN)"};
}
// the sparse-group entries' workspaces: the grouped ones with n doubles of row norms behind them
size_t sgl_carve(size_t grouped, int64_t n, void* base, double** rho) {
  Carver c(base);
  c.take(grouped);
  double* p = static_cast<double*>(c.take(sizeof(double) * (size_t)n));
  if (rho) *rho = p;
  return c.off + 256;
}
void guard_args(const double* rec, const double* out, double mu, double tau, int dtype, int64_t m, int64_t n,
                int64_t l, int64_t max_run, double w_min) {
  if (!rec || !out) throw Error{GLX_E_INVALID, "null argument"};
  check_dims(dtype, n, l);
  check_ratio(tau);
  if (m <= 0) throw Error{GLX_E_INVALID, "m must be positive"};
  if (max_run < 1 || max_run > n) throw Error{GLX_E_INVALID, "max_run must be in 1 .. n"};
  if (!(w_min > 0.0) || !std::isfinite(w_min)) throw Error{GLX_E_INVALID, "w_min must be positive and finite"};
  if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
}

}  // namespace

}  // namespace glx

using namespace glx;

extern "C" {

int glx_group_screen_guard(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l,
                           int64_t max_run, double w_min, double gcol_max, double col_sumsq, double b_norm,
                           double* out) {
  return guarded([&] {
    if (!rec || !out) throw Error{GLX_E_INVALID, "null argument"};
    check_dims(dtype, n, l);
    if (m <= 0) throw Error{GLX_E_INVALID, "m must be positive"};
    if (max_run < 1 || max_run > n) throw Error{GLX_E_INVALID, "max_run must be in 1 .. n"};
    if (!(w_min > 0.0) || !std::isfinite(w_min)) throw Error{GLX_E_INVALID, "w_min must be positive and finite"};
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    group_screen_guard(rec, mu, dtype, m, n, l, max_run, w_min, gcol_max, col_sumsq, b_norm, out);
  });
}

int glx_group_certificate_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (G < 1 || G > n) throw Error{GLX_E_INVALID, "groups: G must be in 1 .. n"};
    *bytes = group_carve(cert_bytes(dtype, m, n, l), G, nullptr, nullptr);
  });
}

int glx_group_certificate_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, char* out,
                                   size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    check_dims(dtype, n, l);
    if (max_run < 1 || max_run > n) throw Error{GLX_E_INVALID, "max_run must be in 1 .. n"};
    const GemmPlan p = a_plan(dtype, m, n, l);
    std::snprintf(out, cap, "A x=%s; A^T r=%s; groups=group kernel (k_group_cert, %s)", plan_field(p, 0).c_str(),
                  plan_field(p, 3).c_str(), group_layout(max_run * l).c_str());
  });
}

int glx_group_certificate(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                          double mu, int64_t G, const int32_t* group_ptr, const double* weights, void* G_out,
                          double* groupnorm_out, double* out, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_dims(dtype, n, l);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    if (!A || !X || !b) throw Error{GLX_E_INVALID, "A, X and b must be device pointers"};
    if (!out) throw Error{GLX_E_INVALID, "null out"};
    const size_t head = cert_bytes(dtype, m, n, l);
    check_workspace(group_carve(head, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                    "glx_group_certificate_workspace_bytes");
    GroupDev d;
    group_carve(head, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupView v = upload(dtype, d, G, group_ptr, weights, f, st);
    certificate_run(dtype, m, n, l, A, X, b, mu, 0, G_out, groupnorm_out, out, d.head, head, stream, &v);
  });
}

int glx_group_certified_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, int screen,
                                        size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (G < 1 || G > n) throw Error{GLX_E_INVALID, "groups: G must be in 1 .. n"};
    *bytes = group_carve(certified_bytes(dtype, m, n, l, screen != 0, G), G, nullptr, nullptr);
  });
}

int glx_group_certified_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, int screen, char* out,
                                 size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    if (max_run < 1 || max_run > n) throw Error{GLX_E_INVALID, "max_run must be in 1 .. n"};
    std::snprintf(out, cap, "%s", certified_describe(dtype, m, n, l, screen != 0, max_run).c_str());
  });
}

int glx_group_certified_solve(const glx_problem* prob, int64_t G, const int32_t* group_ptr, const double* weights,
                              double t, double tol, int64_t maxit, int screen, int check_every,
                              const double* col_norms_dev, const double* col_stats, int32_t* kept_rows_dev,
                              int32_t* kept_groups_dev, void* ws, size_t wsb, glx_group_certified_info* info,
                              void* stream) {
  return guarded([&] {
    if (!prob || !info) throw Error{GLX_E_INVALID, "null problem/info"};
    if (prob->comm != nullptr) throw Error{GLX_E_INVALID, "the certified solve is single-GPU: comm must be NULL"};
    check_dims(prob->dtype, prob->n, prob->l);
    const GroupFacts f = check_groups(prob->n, G, group_ptr, weights);
    const size_t head = certified_bytes(prob->dtype, prob->m, prob->n, prob->l, screen != 0, G);
    check_workspace(group_carve(head, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                    "glx_group_certified_workspace_bytes");
    if (!prob->A || !prob->b || !prob->x) throw Error{GLX_E_INVALID, "A, b and x must be device pointers"};
    GroupDev d;
    group_carve(head, G, ws, &d);
    const GroupView v = upload(prob->dtype, d, G, group_ptr, weights, f, static_cast<hipStream_t>(stream));
    std::memset(info, 0, sizeof *info);
    int64_t listed_groups = 0;
    certified_run(prob, t, tol, maxit, screen, check_every, col_norms_dev, col_stats, kept_rows_dev, d.head, head,
                  &info->base, stream, &v, kept_groups_dev, &listed_groups);
    info->kept_groups = screen != 0 ? info->base.kept : G;
    info->listed_groups = listed_groups;
    info->max_run = f.max_run;
  });
}

/* ---- sample weights (DESIGN.md "Sample weights and cross-validation"): the grouped entries with a
 * weight per row of A; the sums of the weighted finalize sit behind the grouped workspace ---- */

int glx_group_screen_guard_sw(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l,
                              int64_t max_run, double w_min, double gcol_max, double col_sumsq, double b_norm,
                              double* out) {
  return guarded([&] {
    if (!rec || !out) throw Error{GLX_E_INVALID, "null argument"};
    check_dims(dtype, n, l);
    if (m <= 0) throw Error{GLX_E_INVALID, "m must be positive"};
    if (max_run < 1 || max_run > n) throw Error{GLX_E_INVALID, "max_run must be in 1 .. n"};
    if (!(w_min > 0.0) || !std::isfinite(w_min)) throw Error{GLX_E_INVALID, "w_min must be positive and finite"};
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    group_screen_guard(rec, mu, dtype, m, n, l, max_run, w_min, gcol_max, col_sumsq, b_norm, out, true);
  });
}

int glx_group_certificate_sw_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (G < 1 || G > n) throw Error{GLX_E_INVALID, "groups: G must be in 1 .. n"};
    *bytes = sample_bytes(group_carve(cert_bytes(dtype, m, n, l), G, nullptr, nullptr));
  });
}

int glx_group_certificate_sw_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, char* out,
                                      size_t cap) {
  const int rc = glx_group_certificate_describe(dtype, m, n, l, max_run, out, cap);
  if (rc != GLX_OK) return rc;
  const size_t used = std::strlen(out);
  std::snprintf(out + used, cap - used, "; residual=weighted finalize (k_cert_fin_w)");
  return GLX_OK;
}

int glx_group_certificate_sw(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X,
                             const void* b, double mu, int64_t G, const int32_t* group_ptr, const double* weights,
                             const void* sample_w, const void* holdout_w, void* G_out, double* groupnorm_out,
                             double* out, double* holdout_sum, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_dims(dtype, n, l);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    check_sample(sample_w, holdout_w);
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    if (!A || !X || !b) throw Error{GLX_E_INVALID, "A, X and b must be device pointers"};
    if (!out) throw Error{GLX_E_INVALID, "null out"};
    const size_t head = cert_bytes(dtype, m, n, l);
    const size_t grouped = group_carve(head, G, nullptr, nullptr);
    check_workspace(sample_bytes(grouped), ws, wsb, GLX_E_INVALID, "glx_group_certificate_sw_workspace_bytes");
    GroupDev d;
    group_carve(head, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupView v = upload(dtype, d, G, group_ptr, weights, f, st);
    if (holdout_sum != nullptr) *holdout_sum = 0.0;
    if (sample_w == nullptr) {   // today's entry, call for call
      certificate_run(dtype, m, n, l, A, X, b, mu, 0, G_out, groupnorm_out, out, d.head, head, stream, &v);
      return;
    }
    const SampleView sw{sample_w, holdout_w, reinterpret_cast<double*>(static_cast<char*>(ws) + sample_off(grouped))};
    certificate_run(dtype, m, n, l, A, X, b, mu, 0, G_out, groupnorm_out, out, d.head, head, stream, &v, &sw,
                    holdout_sum);
  });
}

int glx_group_certified_sw_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, int screen,
                                           size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (G < 1 || G > n) throw Error{GLX_E_INVALID, "groups: G must be in 1 .. n"};
    *bytes = group_carve(certified_bytes(dtype, m, n, l, screen != 0, G, true), G, nullptr, nullptr);
  });
}

int glx_group_certified_sw_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, int screen,
                                    char* out, size_t cap) {
  const int rc = glx_group_certified_describe(dtype, m, n, l, max_run, screen, out, cap);
  if (rc != GLX_OK) return rc;
  const size_t used = std::strlen(out);
  std::snprintf(out + used, cap - used, "; residual=weighted finalize (k_cert_fin_w)");
  return GLX_OK;
}

int glx_group_certified_solve_sw(const glx_problem* prob, int64_t G, const int32_t* group_ptr, const double* weights,
                                 const void* sample_w, const void* holdout_w, double t, double tol, int64_t maxit,
                                 int screen, int check_every, const double* col_norms_dev, const double* col_stats,
                                 int32_t* kept_rows_dev, int32_t* kept_groups_dev, void* ws, size_t wsb,
                                 glx_group_certified_info* info, double* holdout_sum, void* stream) {
  return guarded([&] {
    if (!prob || !info) throw Error{GLX_E_INVALID, "null problem/info"};
    if (prob->comm != nullptr) throw Error{GLX_E_INVALID, "the certified solve is single-GPU: comm must be NULL"};
    check_dims(prob->dtype, prob->n, prob->l);
    const GroupFacts f = check_groups(prob->n, G, group_ptr, weights);
    check_sample(sample_w, holdout_w);
    const bool weighted = sample_w != nullptr;   // (NULL: the grouped entry's own layout and calls)
    const size_t head = certified_bytes(prob->dtype, prob->m, prob->n, prob->l, screen != 0, G, weighted);
    check_workspace(group_carve(head, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                    "glx_group_certified_sw_workspace_bytes");
    if (!prob->A || !prob->b || !prob->x) throw Error{GLX_E_INVALID, "A, b and x must be device pointers"};
    GroupDev d;
    group_carve(head, G, ws, &d);
    const GroupView v = upload(prob->dtype, d, G, group_ptr, weights, f, static_cast<hipStream_t>(stream));
    std::memset(info, 0, sizeof *info);
    int64_t listed_groups = 0;
    const SampleView sw{sample_w, holdout_w, nullptr};
    certified_run(prob, t, tol, maxit, screen, check_every, col_norms_dev, col_stats, kept_rows_dev, d.head, head,
                  &info->base, stream, &v, kept_groups_dev, &listed_groups, weighted ? &sw : nullptr, holdout_sum);
    info->kept_groups = screen != 0 ? info->base.kept : G;
    info->listed_groups = listed_groups;
    info->max_run = f.max_run;
  });
}

/* ---- the unpenalised intercept (DESIGN.md "Intercept"): the grouped entries; the centring finalize's
 * pieces sit behind the _sw entries' workspaces ---- */

int glx_group_screen_guard_ic(const double* rec, double mu, int dtype, int64_t m, int64_t n, int64_t l,
                              int64_t max_run, double w_min, double gcol_max, const double* col_stats, double b_norm,
                              double weight_sum, double mean_sq, double* out) {
  return guarded([&] {
    if (!rec || !out || !col_stats) throw Error{GLX_E_INVALID, "null argument"};
    check_dims(dtype, n, l);
    if (m <= 0) throw Error{GLX_E_INVALID, "m must be positive"};
    if (max_run < 1 || max_run > n) throw Error{GLX_E_INVALID, "max_run must be in 1 .. n"};
    if (!(w_min > 0.0) || !std::isfinite(w_min)) throw Error{GLX_E_INVALID, "w_min must be positive and finite"};
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    if (!(weight_sum > 0.0) || !std::isfinite(weight_sum))
      throw Error{GLX_E_INVALID, "intercept: weight_sum must be positive and finite"};
    group_screen_guard_ic(rec, mu, dtype, m, n, l, max_run, w_min, gcol_max, col_stats, b_norm, weight_sum, mean_sq,
                          out);
  });
}

int glx_group_certificate_ic_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (G < 1 || G > n) throw Error{GLX_E_INVALID, "groups: G must be in 1 .. n"};
    *bytes = intercept_carve(sample_bytes(group_carve(cert_bytes(dtype, m, n, l), G, nullptr, nullptr)),
                             dtype == GLX_F64 ? 8 : 4, m, l, nullptr, nullptr);
  });
}

int glx_group_certificate_ic_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, char* out,
                                      size_t cap) {
  const int rc = glx_group_certificate_describe(dtype, m, n, l, max_run, out, cap);
  if (rc != GLX_OK) return rc;
  const size_t used = std::strlen(out);
  std::snprintf(out + used, cap - used, "; residual=centring finalize (k_cert_csum, k_cert_fin_c)");
  return GLX_OK;
}

int glx_group_certificate_ic(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X,
                             const void* b, double mu, int64_t G, const int32_t* group_ptr, const double* weights,
                             const void* sample_w, const void* holdout_w, double weight_sum, void* G_out,
                             double* groupnorm_out, double* out, double* holdout_sum, double* intercept_out, void* ws,
                             size_t wsb, void* stream) {
  return guarded([&] {
    check_dims(dtype, n, l);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    check_sample(sample_w, holdout_w);
    check_intercept(weight_sum, intercept_out);
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    if (!A || !X || !b) throw Error{GLX_E_INVALID, "A, X and b must be device pointers"};
    if (!out) throw Error{GLX_E_INVALID, "null out"};
    const int es = dtype == GLX_F64 ? 8 : 4;
    const size_t head = cert_bytes(dtype, m, n, l);
    const size_t grouped = group_carve(head, G, nullptr, nullptr);
    check_workspace(intercept_carve(sample_bytes(grouped), es, m, l, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                    "glx_group_certificate_ic_workspace_bytes");
    GroupDev d;
    group_carve(head, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupView v = upload(dtype, d, G, group_ptr, weights, f, st);
    if (holdout_sum != nullptr) *holdout_sum = 0.0;
    InterceptView ic;
    ic.sigma = weight_sum;
    ic.mean_host = intercept_out;
    intercept_carve(sample_bytes(grouped), es, m, l, ws, &ic);
    const SampleView sw{sample_w, holdout_w, reinterpret_cast<double*>(static_cast<char*>(ws) + sample_off(grouped))};
    certificate_run(dtype, m, n, l, A, X, b, mu, 0, G_out, groupnorm_out, out, d.head, head, stream, &v,
                    sample_w != nullptr ? &sw : nullptr, holdout_sum, &ic);
    for (int64_t c = 0; c < l; ++c) intercept_out[c] = -intercept_out[c];   // c = -r-bar
  });
}

int glx_group_certified_ic_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, int screen,
                                           size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (G < 1 || G > n) throw Error{GLX_E_INVALID, "groups: G must be in 1 .. n"};
    *bytes = group_carve(certified_bytes(dtype, m, n, l, screen != 0, G, true, true), G, nullptr, nullptr);
  });
}

int glx_group_certified_ic_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, int screen,
                                    char* out, size_t cap) {
  const int rc = glx_group_certified_describe(dtype, m, n, l, max_run, screen, out, cap);
  if (rc != GLX_OK) return rc;
  const size_t used = std::strlen(out);
  std::snprintf(out + used, cap - used, "; residual=centring finalize (k_cert_csum, k_cert_fin_c)");
  return GLX_OK;
}

int glx_group_certified_solve_ic(const glx_problem* prob, int64_t G, const int32_t* group_ptr, const double* weights,
                                 const void* sample_w, const void* holdout_w, double weight_sum, double t, double tol,
                                 int64_t maxit, int screen, int check_every, const double* col_norms_dev,
                                 const double* col_stats, int32_t* kept_rows_dev, int32_t* kept_groups_dev, void* ws,
                                 size_t wsb, glx_group_certified_info* info, double* holdout_sum,
                                 double* intercept_out, void* stream) {
  return guarded([&] {
    if (!prob || !info) throw Error{GLX_E_INVALID, "null problem/info"};
    if (prob->comm != nullptr) throw Error{GLX_E_INVALID, "the certified solve is single-GPU: comm must be NULL"};
    check_dims(prob->dtype, prob->n, prob->l);
    const GroupFacts f = check_groups(prob->n, G, group_ptr, weights);
    check_sample(sample_w, holdout_w);
    check_intercept(weight_sum, intercept_out);
    const size_t head = certified_bytes(prob->dtype, prob->m, prob->n, prob->l, screen != 0, G, true, true);
    check_workspace(group_carve(head, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                    "glx_group_certified_ic_workspace_bytes");
    if (!prob->A || !prob->b || !prob->x) throw Error{GLX_E_INVALID, "A, b and x must be device pointers"};
    GroupDev d;
    group_carve(head, G, ws, &d);
    const GroupView v = upload(prob->dtype, d, G, group_ptr, weights, f, static_cast<hipStream_t>(stream));
    std::memset(info, 0, sizeof *info);
    int64_t listed_groups = 0;
    const SampleView sw{sample_w, holdout_w, nullptr};
    InterceptView ic;
    ic.sigma = weight_sum;
    ic.mean_host = intercept_out;
    certified_run(prob, t, tol, maxit, screen, check_every, col_norms_dev, col_stats, kept_rows_dev, d.head, head,
                  &info->base, stream, &v, kept_groups_dev, &listed_groups, sample_w != nullptr ? &sw : nullptr,
                  holdout_sum, &ic);
    for (int64_t c = 0; c < prob->l; ++c) intercept_out[c] = -intercept_out[c];   // c = -r-bar
    info->kept_groups = screen != 0 ? info->base.kept : G;
    info->listed_groups = listed_groups;
    info->max_run = f.max_run;
  });
}

/* ---- one launch at a time ---- */

int glx_group_workspace_bytes(int64_t G, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (G < 1) throw Error{GLX_E_INVALID, "groups: G must be >= 1"};
    *bytes = group_carve(kStepHead, G, nullptr, nullptr);
  });
}

int glx_group_step(int dtype, int64_t n, int64_t rows, int64_t l, int64_t G, const int32_t* group_ptr,
                   const double* weights, const void* y, const void* g, int S, const void* xk, double t, double mu,
                   double thres, double theta, double theta_next, void* xc, void* vnext, void* ynext,
                   void* sums_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_dims(dtype, n, l);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    if (rows < n || rows > n + 63) throw Error{GLX_E_INVALID, "rows must be in n .. n + 63 (the padded width)"};
    if (S < 1 || S > kMaxSplit) throw Error{GLX_E_INVALID, "S must be in 1 .. 64"};
    if (!y || !g || !xk || !xc || !vnext || !ynext || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    check_workspace(group_carve(kStepHead, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_group_workspace_bytes");
    GroupDev d;
    group_carve(kStepHead, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupView v = upload(dtype, d, G, group_ptr, weights, f, st);
    const StepWs w = step_head(d.head);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    const Red red{w.part, w.ticket, static_cast<double*>(sums_dev)};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_group_fista<T>((const T*)y, (const T*)g, S, (const T*)xk, (T*)xc, (T*)vnext, (T*)ynext, v.ptr, v.wts, G,
                            rows, l, v.max_run, t, mu, thres, theta, theta_next, red, st);
    });
    check_launch();
  });
}

int glx_group_certificate_step(int dtype, int64_t n, int64_t l, int64_t G, const int32_t* group_ptr,
                               const double* weights, const void* x, const void* g, int S, double mu, void* gout,
                               double* groupnorm_out, void* sums_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_dims(dtype, n, l);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    if (S < 1 || S > kMaxSplit) throw Error{GLX_E_INVALID, "S must be in 1 .. 64"};
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    if (!x || !g || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    check_workspace(group_carve(kStepHead, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_group_workspace_bytes");
    GroupDev d;
    group_carve(kStepHead, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupView v = upload(dtype, d, G, group_ptr, weights, f, st);
    const StepWs w = step_head(d.head);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    const Red red{w.part, w.ticket, static_cast<double*>(sums_dev)};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_group_cert<T>((const T*)x, (const T*)g, S, (T*)gout, groupnorm_out, v.ptr, v.wts, G, n, l, v.max_run, mu,
                           red, st);
    });
    check_launch();
  });
}

int glx_group_cnorm(int64_t n, int64_t G, const int32_t* group_ptr, const double* weights,
                    const double* col_norms_dev, double* gcn_dev, double* max_dev, void* ws, size_t wsb,
                    void* stream) {
  return guarded([&] {
    check_dims(GLX_F64, n, 1);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    if (!col_norms_dev || !gcn_dev || !max_dev) throw Error{GLX_E_INVALID, "null argument"};
    check_workspace(group_carve(kStepHead, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_group_workspace_bytes");
    GroupDev d;
    group_carve(kStepHead, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupView v = upload(GLX_F64, d, G, group_ptr, weights, f, st);
    const StepWs w = step_head(d.head);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    launch_group_cnorm(col_norms_dev, v.ptr, v.wts, G, v.max_run, gcn_dev, Red{w.part, w.ticket, max_dev}, st);
    check_launch();
  });
}

int glx_group_expand(const int32_t* kept_dev, const int32_t* kept_count_dev, const int32_t* group_ptr_dev,
                     const double* weights_dev, const double* gcn_dev, const int32_t* map_dev, int32_t* rows_out,
                     int32_t* group_ptr_out, double* weights_out, double* gcn_out, int32_t* map_out,
                     int32_t* count_out, void* stream) {
  return guarded([&] {
    if (!kept_dev || !kept_count_dev || !group_ptr_dev || !weights_dev || !gcn_dev || !rows_out || !group_ptr_out ||
        !weights_out || !gcn_out || !map_out || !count_out)
      throw Error{GLX_E_INVALID, "null argument"};
    launch_group_expand(kept_dev, kept_count_dev, group_ptr_dev, weights_dev, gcn_dev, map_dev, rows_out,
                        group_ptr_out, weights_out, gcn_out, map_out, count_out, static_cast<hipStream_t>(stream));
    check_launch();
  });
}

/* ---- the sparse-group lasso (DESIGN.md "Sparse-group lasso"): the grouped entries with a row term,
 * mu (row_ratio sum_i ||x_i|| + (1 - row_ratio) sum_g w_g ||x_[g]||_F). Workspaces: the grouped _sw ones
 * with n doubles of row norms behind them. row_ratio = 0 is the grouped entry's path, call for call ---- */

int glx_sgl_screen_guard(const double* rec, double s_pad, double mu, double row_ratio, int dtype, int64_t m,
                         int64_t n, int64_t l, int64_t max_run, double w_min, double col_max, double col_sumsq,
                         double b_norm, double* out) {
  return guarded([&] {
    guard_args(rec, out, mu, row_ratio, dtype, m, n, l, max_run, w_min);
    sgl_screen_guard(rec, s_pad, mu, row_ratio, dtype, m, n, l, max_run, w_min, col_max, col_sumsq, b_norm, out,
                     false);
  });
}

int glx_sgl_screen_guard_sw(const double* rec, double s_pad, double mu, double row_ratio, int dtype, int64_t m,
                            int64_t n, int64_t l, int64_t max_run, double w_min, double col_max, double col_sumsq,
                            double b_norm, double* out) {
  return guarded([&] {
    guard_args(rec, out, mu, row_ratio, dtype, m, n, l, max_run, w_min);
    sgl_screen_guard(rec, s_pad, mu, row_ratio, dtype, m, n, l, max_run, w_min, col_max, col_sumsq, b_norm, out,
                     true);
  });
}

int glx_sgl_certificate_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (G < 1 || G > n) throw Error{GLX_E_INVALID, "groups: G must be in 1 .. n"};
    *bytes = sgl_carve(sample_bytes(group_carve(cert_bytes(dtype, m, n, l), G, nullptr, nullptr)), n, nullptr, nullptr);
  });
}

int glx_sgl_certificate_describe(int dtype, int64_t m, int64_t n, int64_t l, int weighted, char* out, size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    check_dims(dtype, n, l);
    const GemmPlan p = a_plan(dtype, m, n, l);
    std::snprintf(out, cap, "A x=%s; A^T r=%s; groups=sparse-group kernels (k_sgl_cert, k_sgl_dual_scale: %s)%s",
                  plan_field(p, 0).c_str(), plan_field(p, 3).c_str(), sgl_layout(l).c_str(),
                  weighted != 0 ? "; residual=weighted finalize (k_cert_fin_w)" : "");
  });
}

int glx_sgl_certificate_sw(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                           double mu, double row_ratio, int64_t G, const int32_t* group_ptr, const double* weights,
                           const void* sample_w, const void* holdout_w, void* G_out, double* rownorm_out,
                           double* out, double* holdout_sum, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_dims(dtype, n, l);
    check_ratio(row_ratio);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    check_sample(sample_w, holdout_w);
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    if (!A || !X || !b) throw Error{GLX_E_INVALID, "A, X and b must be device pointers"};
    if (!out) throw Error{GLX_E_INVALID, "null out"};
    const size_t head = cert_bytes(dtype, m, n, l);
    const size_t grouped = group_carve(head, G, nullptr, nullptr);
    check_workspace(sgl_carve(sample_bytes(grouped), n, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                    "glx_sgl_certificate_workspace_bytes");
    GroupDev d;
    group_carve(head, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GroupView v = upload(dtype, d, G, group_ptr, weights, f, st);
    v.row_ratio = row_ratio;
    sgl_carve(sample_bytes(grouped), n, ws, &v.rho);
    for (int k = 8; k < 12; ++k) out[k] = 0.0;
    v.extra = out + 8;
    if (holdout_sum != nullptr) *holdout_sum = 0.0;
    const SampleView sw{sample_w, holdout_w, reinterpret_cast<double*>(static_cast<char*>(ws) + sample_off(grouped))};
    certificate_run(dtype, m, n, l, A, X, b, mu, 0, G_out, rownorm_out, out, d.head, head, stream, &v,
                    sample_w != nullptr ? &sw : nullptr, holdout_sum);
  });
}

int glx_sgl_certificate(int dtype, int64_t m, int64_t n, int64_t l, const void* A, const void* X, const void* b,
                        double mu, double row_ratio, int64_t G, const int32_t* group_ptr, const double* weights,
                        void* G_out, double* rownorm_out, double* out, void* ws, size_t wsb, void* stream) {
  return glx_sgl_certificate_sw(dtype, m, n, l, A, X, b, mu, row_ratio, G, group_ptr, weights, nullptr, nullptr,
                                G_out, rownorm_out, out, nullptr, ws, wsb, stream);
}

int glx_sgl_certified_workspace_bytes(int dtype, int64_t m, int64_t n, int64_t l, int64_t G, int screen,
                                      int weighted, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Error{GLX_E_INVALID, "null bytes"};
    if (G < 1 || G > n) throw Error{GLX_E_INVALID, "groups: G must be in 1 .. n"};
    const size_t head = certified_bytes(dtype, m, n, l, screen != 0, G, weighted != 0, false, true);
    *bytes = sgl_carve(group_carve(head, G, nullptr, nullptr), n, nullptr, nullptr);
  });
}

int glx_sgl_certified_describe(int dtype, int64_t m, int64_t n, int64_t l, int64_t max_run, int screen, int weighted,
                               char* out, size_t cap) {
  return guarded([&] {
    if (!out || cap == 0) throw Error{GLX_E_INVALID, "null out"};
    if (max_run < 1 || max_run > n) throw Error{GLX_E_INVALID, "max_run must be in 1 .. n"};
    std::snprintf(out, cap, "%s%s", certified_describe(dtype, m, n, l, screen != 0, max_run, true).c_str(),
                  weighted != 0 ? "; residual=weighted finalize (k_cert_fin_w)" : "");
  });
}

int glx_sgl_certified_solve_sw(const glx_problem* prob, double row_ratio, int64_t G, const int32_t* group_ptr,
                               const double* weights, const void* sample_w, const void* holdout_w, double t,
                               double tol, int64_t maxit, int screen, int check_every, const double* col_norms_dev,
                               const double* col_stats, int32_t* kept_rows_dev, int32_t* kept_groups_dev, void* ws,
                               size_t wsb, glx_sgl_certified_info* info, double* holdout_sum, void* stream) {
  return guarded([&] {
    if (!prob || !info) throw Error{GLX_E_INVALID, "null problem/info"};
    if (prob->comm != nullptr) throw Error{GLX_E_INVALID, "the certified solve is single-GPU: comm must be NULL"};
    check_dims(prob->dtype, prob->n, prob->l);
    check_ratio(row_ratio);
    const GroupFacts f = check_groups(prob->n, G, group_ptr, weights);
    check_sample(sample_w, holdout_w);
    const bool weighted = sample_w != nullptr;
    const size_t head = certified_bytes(prob->dtype, prob->m, prob->n, prob->l, screen != 0, G, weighted, false, true);
    const size_t grouped = group_carve(head, G, nullptr, nullptr);
    check_workspace(sgl_carve(grouped, prob->n, nullptr, nullptr), ws, wsb, GLX_E_INVALID,
                    "glx_sgl_certified_workspace_bytes");
    if (!prob->A || !prob->b || !prob->x) throw Error{GLX_E_INVALID, "A, b and x must be device pointers"};
    GroupDev d;
    group_carve(head, G, ws, &d);
    GroupView v = upload(prob->dtype, d, G, group_ptr, weights, f, static_cast<hipStream_t>(stream));
    std::memset(info, 0, sizeof *info);
    v.row_ratio = row_ratio;
    v.row_hist = info->kept_row_hist;
    sgl_carve(grouped, prob->n, ws, &v.rho);
    int64_t listed_groups = 0;
    const SampleView sw{sample_w, holdout_w, nullptr};
    // (row_ratio = 0: the grouped solve on a workspace that is merely larger)
    certified_run(prob, t, tol, maxit, screen, check_every, col_norms_dev, col_stats, kept_rows_dev, d.head, head,
                  &info->base.base, stream, &v, kept_groups_dev, &listed_groups, weighted ? &sw : nullptr,
                  holdout_sum);
    info->base.kept_groups = screen != 0 ? info->base.base.kept : G;
    info->base.listed_groups = listed_groups;
    info->base.max_run = f.max_run;
    info->row_ratio = row_ratio;
  });
}

int glx_sgl_certified_solve(const glx_problem* prob, double row_ratio, int64_t G, const int32_t* group_ptr,
                            const double* weights, double t, double tol, int64_t maxit, int screen, int check_every,
                            const double* col_norms_dev, const double* col_stats, int32_t* kept_rows_dev,
                            int32_t* kept_groups_dev, void* ws, size_t wsb, glx_sgl_certified_info* info,
                            void* stream) {
  return glx_sgl_certified_solve_sw(prob, row_ratio, G, group_ptr, weights, nullptr, nullptr, t, tol, maxit, screen,
                                    check_every, col_norms_dev, col_stats, kept_rows_dev, kept_groups_dev, ws, wsb,
                                    info, nullptr, stream);
}

/* ---- one launch at a time (workspace: glx_group_workspace_bytes) ---- */

int glx_sgl_step(int dtype, int64_t n, int64_t rows, int64_t l, int64_t G, const int32_t* group_ptr,
                 const double* weights, const void* y, const void* g, int S, const void* xk, double t, double mu,
                 double row_ratio, double thres, double theta, double theta_next, void* xc, void* vnext, void* ynext,
                 void* sums_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_dims(dtype, n, l);
    check_ratio(row_ratio);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    if (rows < n || rows > n + 63) throw Error{GLX_E_INVALID, "rows must be in n .. n + 63 (the padded width)"};
    if (S < 1 || S > kMaxSplit) throw Error{GLX_E_INVALID, "S must be in 1 .. 64"};
    if (!y || !g || !xk || !xc || !vnext || !ynext || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    check_workspace(group_carve(kStepHead, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_group_workspace_bytes");
    GroupDev d;
    group_carve(kStepHead, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupView v = upload(dtype, d, G, group_ptr, weights, f, st);
    const StepWs w = step_head(d.head);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    const Red red{w.part, w.ticket, static_cast<double*>(sums_dev)};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_sgl_fista<T>((const T*)y, (const T*)g, S, (const T*)xk, (T*)xc, (T*)vnext, (T*)ynext, v.ptr, v.wts, G,
                          rows, l, t, mu, row_ratio, thres, theta, theta_next, red, st);
    });
    check_launch();
  });
}

int glx_sgl_certificate_step(int dtype, int64_t n, int64_t l, int64_t G, const int32_t* group_ptr,
                             const double* weights, const void* x, const void* g, int S, double mu, double row_ratio,
                             void* gout, double* rownorm_out, void* sums_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_dims(dtype, n, l);
    check_ratio(row_ratio);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    if (S < 1 || S > kMaxSplit) throw Error{GLX_E_INVALID, "S must be in 1 .. 64"};
    if (!(mu >= 0.0)) throw Error{GLX_E_INVALID, "mu must be >= 0 (and not NaN)"};
    if (!x || !g || !sums_dev) throw Error{GLX_E_INVALID, "null argument"};
    check_workspace(group_carve(kStepHead, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_group_workspace_bytes");
    GroupDev d;
    group_carve(kStepHead, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupView v = upload(dtype, d, G, group_ptr, weights, f, st);
    const StepWs w = step_head(d.head);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    const Red red{w.part, w.ticket, static_cast<double*>(sums_dev)};
    by_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      launch_sgl_cert<T>((const T*)x, (const T*)g, S, (T*)gout, rownorm_out, v.ptr, v.wts, G, n, l, mu, row_ratio, red,
                         st);
    });
    check_launch();
  });
}

int glx_sgl_dual_scale(int64_t n, int64_t G, const int32_t* group_ptr, const double* weights,
                       const double* rownorms_dev, double a, double cb, double mul0, double add0, double mul1,
                       double add1, double* sg_dev, double* negmin_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_dims(GLX_F64, n, 1);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    if (!rownorms_dev || !negmin_dev) throw Error{GLX_E_INVALID, "null argument"};
    if (!(a >= 0.0) || !(cb >= 0.0)) throw Error{GLX_E_INVALID, "a and cb must be >= 0 (and not NaN)"};
    check_workspace(group_carve(kStepHead, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_group_workspace_bytes");
    GroupDev d;
    group_carve(kStepHead, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupView v = upload(GLX_F64, d, G, group_ptr, weights, f, st);
    const StepWs w = step_head(d.head);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    launch_sgl_dual_scale(rownorms_dev, v.ptr, v.wts, G, a, cb, mul0, add0, mul1, add1, nullptr, sg_dev,
                          Red{w.part, w.ticket, negmin_dev}, st);
    check_launch();
  });
}

int glx_sgl_screen(int64_t n, int64_t G, const int32_t* group_ptr, const double* weights, const double* rownorms_dev,
                   const double* col_norms_dev, const double* gcn_dev, double s, double mul, double add, double rad,
                   double a_lo, double cb_lo, int group_test, int32_t* keep_dev, int32_t* group_keep_dev,
                   double* counts_dev, void* ws, size_t wsb, void* stream) {
  return guarded([&] {
    check_dims(GLX_F64, n, 1);
    const GroupFacts f = check_groups(n, G, group_ptr, weights);
    if (!rownorms_dev || !col_norms_dev || !gcn_dev || !keep_dev || !counts_dev)
      throw Error{GLX_E_INVALID, "null argument"};
    check_workspace(group_carve(kStepHead, G, nullptr, nullptr), ws, wsb, GLX_E_INVALID, "glx_group_workspace_bytes");
    GroupDev d;
    group_carve(kStepHead, G, ws, &d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupView v = upload(GLX_F64, d, G, group_ptr, weights, f, st);
    const StepWs w = step_head(d.head);
    GLX_HIP(hipMemsetAsync(w.ticket, 0, kTicketBytes, st));
    launch_sgl_screen(rownorms_dev, col_norms_dev, gcn_dev, v.ptr, v.wts, G, s, mul, add, nullptr, rad, a_lo, cb_lo,
                      group_test, keep_dev, group_keep_dev, Red{w.part, w.ticket, counts_dev}, st);
    check_launch();
  });
}

int glx_sgl_expand(int64_t G, const int32_t* keep_dev, const int32_t* group_ptr_dev, const double* weights_dev,
                   const double* gcn_dev, const int32_t* map_dev, int32_t* rows_out, int32_t* group_ptr_out,
                   double* weights_out, double* gcn_out, int32_t* map_out, int32_t* count_out, void* stream) {
  return guarded([&] {
    if (G < 1) throw Error{GLX_E_INVALID, "groups: G must be >= 1"};
    if (!keep_dev || !group_ptr_dev || !weights_dev || !gcn_dev || !rows_out || !group_ptr_out || !weights_out ||
        !gcn_out || !map_out || !count_out)
      throw Error{GLX_E_INVALID, "null argument"};
    launch_sgl_expand(keep_dev, group_ptr_dev, weights_dev, gcn_dev, map_dev, G, rows_out, group_ptr_out, weights_out,
                      gcn_out, map_out, count_out, static_cast<hipStream_t>(stream));
    check_launch();
  });
}

}  // extern "C"
