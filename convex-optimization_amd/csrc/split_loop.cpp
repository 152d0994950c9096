// split_loop.cpp — see split_loop.h. Host arithmetic only.
#include "split_loop.h"

#include <cmath>

namespace glx {
namespace split {

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

void SplitTail::begin() {
  trace().clear();
  res->n_fhist = 0;
}

bool SplitTail::step(const double* h) {
  const int ll = (int)(l * l);
  f_now = 0.5 * h[0] + mu * h[1];
  f_best = f_now < f_best ? f_now : f_best;   // min(f_best, f_now): a NaN f_now is not taken
  if (res->f_hist && res->n_fhist < res->f_cap) {
    res->f_hist[res->n_fhist] = f_now;
    if (res->f_hist_best) res->f_hist_best[res->n_fhist] = f_best;
    ++res->n_fhist;
  }
  trace().push_back(h[3] / (double)nl);
  const double rn = spectral_norm(h + kRecHead, (int)l), sn = spectral_norm(h + kRecHead + ll, (int)l);
  if (rn < thres && sn < thres) ++length;
  else length = 0;
  return length >= converge_len;
}

}  // namespace split
}  // namespace glx
