// kernels_admm_primal.hip — the kernels of the primal ADMM solver (reference:
// gl_ADMM_primal.py:47-51, 78-88) between its dense products (Kn w, or K v and g = A^T q, and the
// pass over A):
//   k_admm_primal_w    w = (ATb - z) + rho x, the first iteration's right-hand side (:78)
//   k_admm_primal      the row step (:78-84) on the slabs of the product; it also forms the next
//                      iteration's w (admm_primal_row, glx_device.h)
//   k_admm_primal_fin  sums the slabs of the pass over A into Ax+ (and Az+), reduces
//                      ||Ax+ - b||^2 (:27) and, for the Woodbury form, forms v = A w+
// Expressions keep the reference's evaluation order and scalars are rounded to T first (NEP 50
// weak scalars), as in kernels_admm.hip; reductions are deterministic (grid_reduce, fixed slabs).
#include <cstdlib>

#include "glx.h"
#include "glx_device.h"

namespace glx {

static inline unsigned admm_primal_grid_for(int64_t work, int per_block) {
  int64_t g = (work + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > kMaxBlocks) g = kMaxBlocks;
  return (unsigned)g;
}

template <typename T>
__global__ __launch_bounds__(256) void k_admm_primal_w(const T* __restrict__ ATb, const T* __restrict__ x,
                                                       const T* __restrict__ z, T* __restrict__ w,
                                                       int64_t nl, double rho_) {
  const T rho = (T)rho_;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nl; idx += stride)
    w[idx] = (ATb[idx] - z[idx]) + rho * x[idx];
}

// Rows are owned by LPR lanes holding EPL elements strided by LPR (k_admm_dual's layout). The
// step is row-local and a lane loads all it reads of a row before it stores, so xn, yn, zn, wn
// may be x, y, z, w themselves: those pointers carry no __restrict__.
template <typename T, int LPR, int EPL, bool WOODBURY>
__global__ __launch_bounds__(256) void k_admm_primal(const T* __restrict__ prod, int S, const T* x,
                                                     const T* y, const T* z, const T* w,
                                                     const T* __restrict__ ATb, T* xn, T* yn, T* zn,
                                                     T* __restrict__ rn, T* __restrict__ sn, T* wn,
                                                     int64_t n, int64_t l, AdmmPrimalScalars sc, Red red) {
  const T rho = (T)sc.rho, etarho = (T)sc.etarho, etamu = (T)sc.etamu, taurho = (T)sc.taurho;
  const T thres = (T)sc.thres;
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
    T pv[EPL], xv[EPL], yv[EPL], zv[EPL], wv[EPL], av[EPL];
    bool ok[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPR;
      ok[e] = rv && j < l;
      pv[e] = ok[e] ? slab_sum(prod, S, nl, base + j) : T(0);
      xv[e] = ok[e] ? x[base + j] : T(0);
      yv[e] = ok[e] ? y[base + j] : T(0);
      zv[e] = ok[e] ? z[base + j] : T(0);
      wv[e] = (WOODBURY && ok[e]) ? w[base + j] : T(0);
      av[e] = ok[e] ? ATb[base + j] : T(0);
    }
    AdmmPrimalRow<T, EPL> o;
    admm_primal_row<T, LPR, EPL, WOODBURY>(pv, xv, yv, zv, wv, av, ok, rv, sub, rho, etarho, etamu, taurho,
                                           thres, o, acc);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPR;
      if (ok[e]) {
        xn[base + j] = o.x[e];
        yn[base + j] = o.y[e];
        zn[base + j] = o.z[e];
        rn[base + j] = o.r[e];
        sn[base + j] = o.s[e];
        wn[base + j] = o.w[e];
      }
    }
  }
  grid_reduce<2, 0x2u>(acc, red);
}

template <typename T>
__global__ __launch_bounds__(256) void k_admm_primal_fin(const T* __restrict__ P, int S,
                                                         const T* __restrict__ b,
                                                         const T* __restrict__ AATb, T* __restrict__ Ax,
                                                         T* __restrict__ Az, T* __restrict__ v,
                                                         int64_t ml, double rho_, Red red) {
  const T rho = (T)rho_;
  double acc[1] = {0.0};
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ml; idx += stride) {
    const T ax = slab_sum(P, S, ml, idx);
    Ax[idx] = ax;
    if (AATb != nullptr) {   // uniform over the grid
      const T az = slab_sum(P + (int64_t)S * ml, S, ml, idx);
      Az[idx] = az;
      v[idx] = (AATb[idx] - az) + rho * ax;
    }
    const T r = ax - b[idx];
    acc[0] += (double)(r * r);
  }
  grid_reduce<1, 0u>(acc, red);
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
template <typename T>
void launch_admm_primal_w(const T* ATb, const T* x, const T* z, T* w, int64_t nl, double rho, hipStream_t st) {
  hipLaunchKernelGGL(k_admm_primal_w<T>, dim3(admm_primal_grid_for(nl, 256 * 4)), dim3(256), 0, st, ATb, x, z,
                     w, nl, rho);
}

template <typename T, int LPR, int EPL>
static void admm_primal_go(bool woodbury, const T* prod, int S, const T* x, const T* y, const T* z,
                           const T* w, const T* ATb, T* xn, T* yn, T* zn, T* rn, T* sn, T* wn, int64_t n,
                           int64_t l, const AdmmPrimalScalars& sc, Red red, hipStream_t st) {
  unsigned grid = admm_primal_grid_for(n, 256 / LPR);
  if (grid > 512u) grid = 512u;   // two trips per workgroup at n = 16384 (kernels_elem.hip kRowBlocks)
  if (woodbury)
    hipLaunchKernelGGL((k_admm_primal<T, LPR, EPL, true>), dim3(grid), dim3(256), 0, st, prod, S, x, y, z, w,
                       ATb, xn, yn, zn, rn, sn, wn, n, l, sc, red);
  else
    hipLaunchKernelGGL((k_admm_primal<T, LPR, EPL, false>), dim3(grid), dim3(256), 0, st, prod, S, x, y, z, w,
                       ATb, xn, yn, zn, rn, sn, wn, n, l, sc, red);
}
template <typename T>
void launch_admm_primal(bool woodbury, const T* prod, int S, const T* x, const T* y, const T* z, const T* w,
                        const T* ATb, T* xn, T* yn, T* zn, T* rn, T* sn, T* wn, int64_t n, int64_t l,
                        const AdmmPrimalScalars& sc, Red red, hipStream_t st) {
#define GLX_ADMM_GO(LPR, EPL) \
  admm_primal_go<T, LPR, EPL>(woodbury, prod, S, x, y, z, w, ATb, xn, yn, zn, rn, sn, wn, n, l, sc, red, st)
  if (l <= 1) GLX_ADMM_GO(1, 1);
  else if (l <= 2) GLX_ADMM_GO(2, 1);
  else if (l <= 4) GLX_ADMM_GO(4, 1);
  else if (l <= 8) GLX_ADMM_GO(8, 1);
  else if (l <= 16) GLX_ADMM_GO(16, 1);
  else if (l <= 32) GLX_ADMM_GO(16, 2);
  else throw Error{GLX_E_INVALID, "the primal ADMM row step takes l <= 32"};
#undef GLX_ADMM_GO
}

template <typename T>
void launch_admm_primal_fin(const T* P, int S, const T* b, const T* AATb, T* Ax, T* Az, T* v, int64_t ml,
                            double rho, Red red, hipStream_t st) {
  hipLaunchKernelGGL(k_admm_primal_fin<T>, dim3(admm_primal_grid_for(ml, 256)), dim3(256), 0, st, P, S, b,
                     AATb, Ax, Az, v, ml, rho, red);
}

#define GLX_ADMM_PRIMAL_INST(T)                                                                          \
  template void launch_admm_primal_w<T>(const T*, const T*, const T*, T*, int64_t, double, hipStream_t); \
  template void launch_admm_primal<T>(bool, const T*, int, const T*, const T*, const T*, const T*,       \
                                      const T*, T*, T*, T*, T*, T*, T*, int64_t, int64_t,                \
                                      const AdmmPrimalScalars&, Red, hipStream_t);                       \
  template void launch_admm_primal_fin<T>(const T*, int, const T*, const T*, T*, T*, T*, int64_t, double, \
                                          Red, hipStream_t);

GLX_ADMM_PRIMAL_INST(double)
GLX_ADMM_PRIMAL_INST(float)

}  // namespace glx
