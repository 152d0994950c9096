// kernels_admm.hip — the kernels of the dual ADMM solver (reference: gl_ADMM_dual.py:61-93)
// between its three dense products z = K v, g = A^T z and A @ [x+ | u+]:
//   k_admm_v     v = (Ax - rho Au) - b, the right-hand side of the K product (:63)
//   k_admm_dual  the row step (:64-67) on a given g (its fused form is k_atr_admm, kernels_atr.hip;
//                both run admm_dual_row, glx_device.h)
//   k_admm_fin   sums the batched pass's slabs into Ax+ and Au+, forms s = Au - Au+ (:68) and
//                reduces ||Ax+ - b||^2 (:26)
//   k_gram       R^T R in double for the spectral norms of the stop rule (:85-86), two stages
// Expressions keep the reference's evaluation order and scalars are rounded to T first (NEP 50
// weak scalars), as in kernels_elem.hip; reductions are deterministic (grid_reduce, fixed slabs).
#include <cstdlib>

#include "glx.h"
#include "glx_device.h"

namespace glx {

static inline unsigned admm_grid_for(int64_t work, int per_block) {
  int64_t g = (work + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > kMaxBlocks) g = kMaxBlocks;
  return (unsigned)g;
}

template <typename T>
__global__ __launch_bounds__(256) void k_admm_v(const T* __restrict__ Ax, const T* __restrict__ Au,
                                                const T* __restrict__ b, T* __restrict__ v, int64_t ml,
                                                double rho_) {
  const T rho = (T)rho_;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ml; idx += stride)
    v[idx] = (Ax[idx] - rho * Au[idx]) - b[idx];
}

// Rows of x are owned by LPR lanes holding EPL elements strided by LPR (kernels_elem.hip's layout)
template <typename T, int LPR, int EPL>
__global__ __launch_bounds__(256) void k_admm_dual(const T* __restrict__ x, const T* __restrict__ g, int S,
                                                   T* __restrict__ gout, T* __restrict__ un,
                                                   T* __restrict__ xn, T* __restrict__ rn, int64_t n,
                                                   int64_t l, double rho_, double taurho_, double mu_,
                                                   Red red) {
  const T rho = (T)rho_, taurho = (T)taurho_, mu = (T)mu_;
  const int64_t nl = n * l;
  double acc[2] = {0.0, -__builtin_inf()};
  const int sub = threadIdx.x & (LPR - 1);
  const int64_t rows_per_block = 256 / LPR;
  const int64_t row_stride = (int64_t)gridDim.x * rows_per_block;
  const int64_t n_trips = (n + row_stride - 1) / row_stride;
  for (int64_t trip = 0; trip < n_trips; ++trip) {   // uniform trip count: every lane shuffles
    const int64_t row = trip * row_stride + (int64_t)blockIdx.x * rows_per_block + (threadIdx.x / LPR);
    const bool rv = row < n;
    const int64_t base = (rv ? row : 0) * l;
    T xv[EPL], gv[EPL], uv[EPL], xo[EPL], rr[EPL];
    bool ok[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPR;
      ok[e] = rv && j < l;
      xv[e] = ok[e] ? x[base + j] : T(0);
      gv[e] = ok[e] ? slab_sum(g, S, nl, base + j) : T(0);
      if (ok[e] && gout != nullptr) gout[base + j] = gv[e];
    }
    admm_dual_row<T, LPR, EPL>(xv, gv, ok, rv, sub, rho, taurho, mu, uv, xo, rr, acc);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPR;
      if (ok[e]) {
        un[base + j] = uv[e];
        xn[base + j] = xo[e];
        rn[base + j] = rr[e];
      }
    }
  }
  grid_reduce<2, 0x2u>(acc, red);
}

template <typename T>
__global__ __launch_bounds__(256) void k_admm_fin(const T* __restrict__ P, int S, const T* __restrict__ b,
                                                  T* __restrict__ Ax, T* __restrict__ Au,
                                                  T* __restrict__ s, int64_t ml, Red red) {
  double v[1] = {0.0};
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ml; idx += stride) {
    const T ax = slab_sum(P, S, ml, idx);
    const T au = slab_sum(P + (int64_t)S * ml, S, ml, idx);
    if (s != nullptr) s[idx] = Au[idx] - au;
    Ax[idx] = ax;
    Au[idx] = au;
    const T r = ax - b[idx];
    v[0] += (double)(r * r);
  }
  grid_reduce<1, 0u>(v, red);
}

// Stage 1 of R^T R: workgroup `blk` of nb owns the rows [rows blk / nb, rows (blk + 1) / nb), staged
// through LDS kGramRows at a time as doubles; thread t accumulates the entries t, t + 256, ...
// (< l * l <= 1024) over the rows in ascending order.
constexpr int kGramRows = 64;
constexpr int kGramMaxL = 32;
template <typename T>
__global__ __launch_bounds__(256) void k_gram(const T* __restrict__ R, int64_t rows, int l,
                                              double* __restrict__ part) {
  __shared__ double sh[kGramRows][kGramMaxL + 1];
  const int ll = l * l;
  const int64_t rb = rows * (int64_t)blockIdx.x / gridDim.x, re = rows * ((int64_t)blockIdx.x + 1) / gridDim.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  int ei[4], ej[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = (int)threadIdx.x + 256 * q;
    ei[q] = e < ll ? e / l : 0;
    ej[q] = e < ll ? e % l : 0;
  }
  for (int64_t r0 = rb; r0 < re; r0 += kGramRows) {
    const int cnt = (int)(re - r0 < kGramRows ? re - r0 : kGramRows);
    for (int t = threadIdx.x; t < cnt * l; t += 256) sh[t / l][t % l] = (double)R[r0 * l + t];
    __syncthreads();
    for (int r = 0; r < cnt; ++r) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = acc[q] + sh[r][ei[q]] * sh[r][ej[q]];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = (int)threadIdx.x + 256 * q;
    if (e < ll) part[(int64_t)blockIdx.x * ll + e] = acc[q];
  }
}
// Stage 2: entry e = the sum of the nb partials in slab order
__global__ __launch_bounds__(256) void k_gram_sum(const double* __restrict__ part, int nb, int ll,
                                                  double* __restrict__ gram) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= ll) return;
  double v = part[e];
  for (int k = 1; k < nb; ++k) v = v + part[(int64_t)k * ll + e];
  gram[e] = v;
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
template <typename T>
void launch_admm_v(const T* Ax, const T* Au, const T* b, T* v, int64_t ml, double rho, hipStream_t st) {
  hipLaunchKernelGGL(k_admm_v<T>, dim3(admm_grid_for(ml, 256 * 4)), dim3(256), 0, st, Ax, Au, b, v, ml, rho);
}

template <typename T, int LPR, int EPL>
static void admm_dual_go(const T* x, const T* g, int S, T* gout, T* un, T* xn, T* rn, int64_t n, int64_t l,
                         double rho, double taurho, double mu, Red red, hipStream_t st) {
  unsigned grid = admm_grid_for(n, 256 / LPR);
  if (grid > 512u) grid = 512u;   // two trips per workgroup at n = 16384 (kernels_elem.hip kRowBlocks)
  hipLaunchKernelGGL((k_admm_dual<T, LPR, EPL>), dim3(grid), dim3(256), 0, st, x, g, S, gout, un, xn, rn, n,
                     l, rho, taurho, mu, red);
}
template <typename T>
void launch_admm_dual(const T* x, const T* g, int S, T* gout, T* un, T* xn, T* rn, int64_t n, int64_t l,
                      double rho, double taurho, double mu, Red red, hipStream_t st) {
#define GLX_ADMM_GO(LPR, EPL) \
  admm_dual_go<T, LPR, EPL>(x, g, S, gout, un, xn, rn, n, l, rho, taurho, mu, red, st)
  if (l <= 1) GLX_ADMM_GO(1, 1);
  else if (l <= 2) GLX_ADMM_GO(2, 1);
  else if (l <= 4) GLX_ADMM_GO(4, 1);
  else if (l <= 8) GLX_ADMM_GO(8, 1);
  else if (l <= 16) GLX_ADMM_GO(16, 1);
  else if (l <= 32) GLX_ADMM_GO(16, 2);
  else throw Error{GLX_E_INVALID, "the dual ADMM row step takes l <= 32"};
#undef GLX_ADMM_GO
}

template <typename T>
void launch_admm_fin(const T* P, int S, const T* b, T* Ax, T* Au, T* s, int64_t ml, Red red,
                     hipStream_t st) {
  hipLaunchKernelGGL(k_admm_fin<T>, dim3(admm_grid_for(ml, 256)), dim3(256), 0, st, P, S, b, Ax, Au, s, ml, red);
}

int gram_blocks(int64_t rows) {
  const int64_t g = (rows + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 256 ? 256 : g));
}
template <typename T>
void launch_gram(const T* R, int64_t rows, int64_t l, double* part, double* gram, hipStream_t st) {
  if (l < 1 || l > kGramMaxL) throw Error{GLX_E_INVALID, "the Gram kernel takes 1 <= l <= 32"};
  const int nb = gram_blocks(rows), ll = (int)(l * l);
  hipLaunchKernelGGL(k_gram<T>, dim3(nb), dim3(256), 0, st, R, rows, (int)l, part);
  hipLaunchKernelGGL(k_gram_sum, dim3((ll + 255) / 256), dim3(256), 0, st, part, nb, ll, gram);
}

#define GLX_ADMM_INST(T)                                                                           \
  template void launch_admm_v<T>(const T*, const T*, const T*, T*, int64_t, double, hipStream_t);  \
  template void launch_admm_dual<T>(const T*, const T*, int, T*, T*, T*, T*, int64_t, int64_t,     \
                                    double, double, double, Red, hipStream_t);                     \
  template void launch_admm_fin<T>(const T*, int, const T*, T*, T*, T*, int64_t, Red, hipStream_t); \
  template void launch_gram<T>(const T*, int64_t, int64_t, double*, double*, hipStream_t);

GLX_ADMM_INST(double)
GLX_ADMM_INST(float)

}  // namespace glx
