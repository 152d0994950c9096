// kernels_alm.hip — the kernels of the dual ALM solver (reference: gl_ALM_dual.py:10-63, 116-124)
// beside its dense products:
//   k_alm_inner  one step of the inner Nesterov loop on a given P = Qn y, any n and l <= 32 (its
//                fused form is k_atr_alm, its panel form k_alm_inner_panel, kernels_atr.hip; all
//                three run alm_inner_row, glx_device.h)
//   k_alm_j      J = rho (A^T E - x / rho), the linear term of the subproblem's gradient (:38, with
//                J = rho H; DESIGN.md, "Dual ALM")
//   k_alm_x      r = u + A^T z, x+ = x - (tau rho) r (:121-123) and the objective's row sums
// Expressions keep the reference's evaluation order, as in kernels_admm.hip. fp64 only.
#include <cstdlib>

#include "glx.h"
#include "glx_device.h"

namespace glx {

static inline unsigned alm_grid_for(int64_t work, int per_block, int cap) {
  int64_t g = (work + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

// Rows are owned by LPR lanes holding EPL elements strided by LPR (kernels_elem.hip's layout)
template <typename T, int LPR, int EPL>
__global__ __launch_bounds__(256) void k_alm_inner(const T* __restrict__ P, int S, const T* __restrict__ y,
                                                   const T* __restrict__ J, const T* u, T* un,
                                                   T* __restrict__ yn, int64_t n, int64_t l, T t, T mu,
                                                   T gamma, T a1, T gn) {
  const int64_t nl = n * l;
  const int sub = threadIdx.x & (LPR - 1);
  const int64_t rows_per_block = 256 / LPR;
  const int64_t row_stride = (int64_t)gridDim.x * rows_per_block;
  const int64_t n_trips = (n + row_stride - 1) / row_stride;
  for (int64_t trip = 0; trip < n_trips; ++trip) {   // uniform trip count: every lane shuffles
    const int64_t row = trip * row_stride + (int64_t)blockIdx.x * rows_per_block + (threadIdx.x / LPR);
    const bool rv = row < n;
    const int64_t base = (rv ? row : 0) * l;
    T pv[EPL], yv[EPL], jv[EPL], uv[EPL], uo[EPL], yo[EPL];
    bool ok[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPR;
      ok[e] = rv && j < l;
      pv[e] = ok[e] ? slab_sum(P, S, nl, base + j) : T(0);
      yv[e] = ok[e] ? y[base + j] : T(0);
      jv[e] = ok[e] ? J[base + j] : T(0);
      uv[e] = ok[e] ? u[base + j] : T(0);
    }
    alm_inner_row<T, LPR, EPL>(pv, yv, jv, uv, t, mu, gamma, a1, gn, uo, yo);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPR;
      if (ok[e]) {
        un[base + j] = uo[e];
        if (yn != nullptr) yn[base + j] = yo[e];
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_alm_j(const T* __restrict__ h, int S, const T* __restrict__ x,
                                               T* __restrict__ J, int64_t nl, T rho) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nl; idx += stride)
    J[idx] = rho * (slab_sum(h, S, nl, idx) - x[idx] / rho);
}

template <typename T, int LPR, int EPL>
__global__ __launch_bounds__(256) void k_alm_x(const T* x, const T* __restrict__ u, const T* __restrict__ g,
                                               int S, T* xn, T* __restrict__ rn, int64_t n, int64_t l,
                                               T taurho, Red red) {
  const int64_t nl = n * l;
  double acc[2] = {0.0, -__builtin_inf()};
  const int sub = threadIdx.x & (LPR - 1);
  const int64_t rows_per_block = 256 / LPR;
  const int64_t row_stride = (int64_t)gridDim.x * rows_per_block;
  const int64_t n_trips = (n + row_stride - 1) / row_stride;
  for (int64_t trip = 0; trip < n_trips; ++trip) {
    const int64_t row = trip * row_stride + (int64_t)blockIdx.x * rows_per_block + (threadIdx.x / LPR);
    const bool rv = row < n;
    const int64_t base = (rv ? row : 0) * l;
    T xsq = T(0);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPR;
      if (rv && j < l) {
        const T r = u[base + j] + slab_sum(g, S, nl, base + j);
        const T xo = x[base + j] - taurho * r;
        rn[base + j] = r;
        xn[base + j] = xo;
        acc[1] = nan_max(acc[1], (double)tabs(xo));
        xsq = xsq + xo * xo;
      }
    }
    const T xnorm = __builtin_sqrt(row_allsum<LPR>(xsq));
    if (rv && sub == 0) acc[0] += (double)xnorm;
  }
  grid_reduce<2, 0x2u>(acc, red);
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
template <typename T>
void launch_alm_inner(const T* P, int S, const T* y, const T* J, const T* u, T* un, T* yn, int64_t n,
                      int64_t l, double t, double mu, double gamma, double gamma_next, hipStream_t st) {
#define GLX_ALM_GO(LPR, EPL)                                                                          \
  hipLaunchKernelGGL((k_alm_inner<T, LPR, EPL>), dim3(alm_grid_for(n, 256 / LPR, 512)), dim3(256), 0, st, P, \
                     S, y, J, u, un, yn, n, l, (T)t, (T)mu, (T)gamma, (T)(1.0 - gamma_next), (T)gamma_next)
  if (l <= 1) GLX_ALM_GO(1, 1);
  else if (l <= 2) GLX_ALM_GO(2, 1);
  else if (l <= 4) GLX_ALM_GO(4, 1);
  else if (l <= 8) GLX_ALM_GO(8, 1);
  else if (l <= 16) GLX_ALM_GO(16, 1);
  else if (l <= 32) GLX_ALM_GO(16, 2);
  else throw Error{GLX_E_INVALID, "the dual ALM inner step takes l <= 32"};
#undef GLX_ALM_GO
}

template <typename T>
void launch_alm_j(const T* h, int S, const T* x, T* J, int64_t nl, double rho, hipStream_t st) {
  hipLaunchKernelGGL(k_alm_j<T>, dim3(alm_grid_for(nl, 256 * 4, kMaxBlocks)), dim3(256), 0, st, h, S, x, J, nl,
                     (T)rho);
}

template <typename T>
void launch_alm_x(const T* x, const T* u, const T* g, int S, T* xn, T* rn, int64_t n, int64_t l,
                  double taurho, Red red, hipStream_t st) {
#define GLX_ALM_GO(LPR, EPL)                                                                            \
  hipLaunchKernelGGL((k_alm_x<T, LPR, EPL>), dim3(alm_grid_for(n, 256 / LPR, 512)), dim3(256), 0, st, x, u, g, \
                     S, xn, rn, n, l, (T)taurho, red)
  if (l <= 1) GLX_ALM_GO(1, 1);
  else if (l <= 2) GLX_ALM_GO(2, 1);
  else if (l <= 4) GLX_ALM_GO(4, 1);
  else if (l <= 8) GLX_ALM_GO(8, 1);
  else if (l <= 16) GLX_ALM_GO(16, 1);
  else if (l <= 32) GLX_ALM_GO(16, 2);
  else throw Error{GLX_E_INVALID, "the dual ALM x update takes l <= 32"};
#undef GLX_ALM_GO
}

template void launch_alm_inner<double>(const double*, int, const double*, const double*, const double*,
                                       double*, double*, int64_t, int64_t, double, double, double, double,
                                       hipStream_t);
template void launch_alm_j<double>(const double*, int, const double*, double*, int64_t, double, hipStream_t);
template void launch_alm_x<double>(const double*, const double*, const double*, int, double*, double*,
                                   int64_t, int64_t, double, Red, hipStream_t);

}  // namespace glx
