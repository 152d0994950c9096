// split_loop.h — the host arithmetic the three split solvers (dual ADMM, primal ADMM, dual ALM)
// share after each outer iteration's readback. Nothing here or in split_loop.cpp calls or includes
// HIP, so the unit builds and runs on its own (tests/test_host_cpu.py); the copies and waits around
// it are glx_host.h's SplitLoop.
#pragma once

#include <stdint.h>

#include <limits>
#include <vector>

#include "glx.h"

namespace glx {
namespace split {

constexpr int kMaxL = 32;    // the Gram kernel and the host Jacobi sweep
constexpr int kRecHead = 4;  // record: [||Ax - b||^2, sum_i ||x_i||, max |x|, count] + 2 Grams

// largest eigenvalue of the symmetric l x l matrix G (row-major, l <= kMaxL) by cyclic Jacobi
// sweeps, NaN where G holds one; the spectral norm of R from gram = R^T R
double sym_lambda_max(const double* G, int l);
double spectral_norm(const double* gram, int l);
// sparsity of the iterate after each iteration of this thread's last solve (glx_admm_trace)
std::vector<double>& trace();

// One solve's objective, histories and stop rule (gl_ADMM_dual.py:85-93 and its two siblings).
struct SplitTail {
  double mu, thres;
  int64_t converge_len, nl, l;
  glx_result* res;   // f_hist / f_hist_best (may be NULL) under f_cap, n_fhist
  double f_now = 0.0, f_best = std::numeric_limits<double>::infinity();
  int64_t length = 0;   // iterations in a row with both spectral norms under thres

  void begin();   // clears the trace and the history count
  // h = an iteration's record: f_now = 0.5 h[0] + mu h[1]; f_best takes it unless it is NaN; both
  // go to the histories while there is room; h[3] / nl to the trace; the streak grows when
  // ||r||_2 and ||s||_2 (from the two Gram matrices) are both < thres, else restarts. True: stop.
  bool step(const double* h);
};

}  // namespace split
}  // namespace glx
