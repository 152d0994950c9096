// kernels_cert.hip — the kernels of the optimality certificate (DESIGN.md "Certificate") around
// its two dense products A x and g = A^T r:
//   k_cert_fin  sums the slabs of A x in slab order into r = A x - b and reduces ||r||^2, <r, b>
//   k_cert_fin_w  the same with one weight per row of A: r, w r and the weighted sums
//   k_cert_csum / k_cert_fin_c  the same for the problem with an intercept: r and its weighted column
//               means, then the centred residual, w times it and the sums on it
//   k_cert_row the row terms (cert_row, glx_device.h) on a given g, any n and l <= kMaxL (their
//               fused form is k_atr_cert and its panel counterpart k_cert_panel, kernels_atr.hip)
// mu is rounded to T first, as in kernels_elem.hip; reductions are deterministic (grid_reduce,
// fixed slabs) and accumulate in double.
#include <cstdlib>
#include <type_traits>

#include "glx.h"
#include "glx_device.h"

namespace glx {

static inline unsigned cert_grid_for(int64_t work, int per_block) {
  int64_t g = (work + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > kMaxBlocks) g = kMaxBlocks;
  return (unsigned)g;
}

template <typename T>
__global__ __launch_bounds__(256) void k_cert_fin(const T* __restrict__ P, int S, const T* __restrict__ b,
                                                  T* __restrict__ r, int64_t ml, Red red) {
  double v[2] = {0.0, 0.0};
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ml; idx += stride) {
    const T ax = S > 0 ? slab_sum(P, S, ml, idx) : T(0);
    const T bv = b[idx];
    const T rv = ax - bv;
    r[idx] = rv;
    v[0] += (double)rv * (double)rv;
    v[1] += (double)rv * (double)bv;
  }
  grid_reduce<2, 0u>(v, red);
}

// The finalize of the sample-weighted problem (DESIGN.md "Sample weights and cross-validation"):
// k_cert_fin's thread-to-element map and accumulation order with one weight per row of A (element
// idx belongs to row idx / l; w holds m values of T, >= 0). r (may be NULL) receives the unweighted
// r^ = fl(A x) - b, rw = fl(w r^) is the operand of the A^T pass, and the sums are
//   [sum w r^2, sum w r^ b, sum v r^2 (HOLD: v = the hold-out weights)]
// with every product formed as ((double)w r^) r^, which is exact for w = 1: the first two sums and rw
// are then k_cert_fin's bits. The row comes from a plain division, 32-bit where m l allows it: at one
// element per thread it is noise beside the loads (the launch is a few microseconds between two
// passes over A).
template <typename T, bool HOLD>
__global__ __launch_bounds__(256) void k_cert_fin_w(const T* __restrict__ P, int S, const T* __restrict__ b,
                                                    const T* __restrict__ w, const T* __restrict__ hv,
                                                    T* __restrict__ r, T* __restrict__ rw, int64_t ml, int64_t l,
                                                    Red red) {
  double v[HOLD ? 3 : 2] = {};
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool narrow = ml <= (int64_t)0xffffffffll;   // uniform: l <= ml
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ml; idx += stride) {
    const int64_t row = narrow ? (int64_t)((unsigned)idx / (unsigned)l) : idx / l;
    const T ax = S > 0 ? slab_sum(P, S, ml, idx) : T(0);
    const T bv = b[idx];
    const T wv = w[row];
    const T rv = ax - bv;
    if (r != nullptr) r[idx] = rv;
    rw[idx] = wv * rv;
    const double wr = (double)wv * (double)rv;
    v[0] += wr * (double)rv;
    v[1] += wr * (double)bv;
    if constexpr (HOLD) v[2] += ((double)hv[row] * (double)rv) * (double)rv;
  }
  grid_reduce<HOLD ? 3 : 2, 0u>(v, red);
}

// ------------------------------------------------------------------------------------------
// The centring finalize of the problem with an unpenalised intercept (DESIGN.md "Intercept"):
// two launches between the two dense passes, siblings of the finalizes above.
//   k_cert_csum   r^ = fl(A y) - b (the slabs summed as in k_cert_fin) and the l weighted column
//                 means  mean[c] = sum_j w_j r^_jc / sigma  (w == NULL: unit weights)
//   k_cert_fin_c  r_c = (T)((double)r^ - mean[c]), rw = fl(w r_c) and the sums of k_cert_fin_w on r_c
// ------------------------------------------------------------------------------------------
// The workgroup is a 2-D thread map of 256 >> cx_log rows by CX = 1 << cx_log columns, CX the power of
// two >= l (lanes with tx >= l are masked), so the element-to-column map holds for every l <= 128 and
// a row's l values are read by adjacent lanes. A thread adds its rows in row order; the rows of a
// workgroup combine through an in-order balanced tree over ty in shared memory; the workgroups'
// partials (write-through stores, an integer arrival counter, as k_col_norms) are combined by the
// last to arrive: thread (ty, tx) adds a contiguous run of workgroups in workgroup order, the runs
// combine through the same tree in run order. Every order is a function of (m, l) alone.
constexpr int kCsumBlocks = 256;
size_t cert_csum_part_bytes() { return sizeof(double) * (size_t)kCsumBlocks * (size_t)kMaxL; }

template <typename T>
__global__ __launch_bounds__(256) void k_cert_csum(const T* __restrict__ P, int S, const T* __restrict__ b,
                                                   const T* __restrict__ w, T* __restrict__ rh, int64_t m, int64_t l,
                                                   int cx_log, double sigma, double* __restrict__ part,
                                                   unsigned* __restrict__ cnt, double* __restrict__ mean) {
  __shared__ double sh[256];
  __shared__ int last;
  const int CX = 1 << cx_log, RY = 256 >> cx_log;
  const int tx = threadIdx.x & (CX - 1), ty = threadIdx.x >> cx_log;
  const bool colok = tx < l;
  const int64_t ml = m * l;
  double acc = 0.0;
  if (colok) {
    for (int64_t row = (int64_t)blockIdx.x * RY + ty; row < m; row += (int64_t)gridDim.x * RY) {
      const int64_t idx = row * l + tx;
      const T ax = S > 0 ? slab_sum(P, S, ml, idx) : T(0);
      const T rv = ax - b[idx];
      rh[idx] = rv;
      acc += (w != nullptr ? (double)w[row] : 1.0) * (double)rv;
    }
  }
  sh[threadIdx.x] = acc;   // (threadIdx.x = ty CX + tx)
  __syncthreads();
  for (int s = 1; s < RY; s <<= 1) {
    if ((ty & (2 * s - 1)) == 0) sh[threadIdx.x] += sh[threadIdx.x + s * CX];
    __syncthreads();
  }
  if (ty == 0 && colok)
    __hip_atomic_store(part + (int64_t)blockIdx.x * l + tx, sh[tx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // write-through stores drained before the arrival (kernels_screen.hip k_col_norms)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned arrival = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = arrival == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  const int nb = (int)gridDim.x;
  const int run = (nb + RY - 1) / RY;
  const int k0 = ty * run < nb ? ty * run : nb;
  const int k1 = k0 + run < nb ? k0 + run : nb;
  double s = 0.0;
  if (colok) {
#pragma unroll 8
    for (int k = k0; k < k1; ++k)
      s += __hip_atomic_load(part + (int64_t)k * l + tx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int st = 1; st < RY; st <<= 1) {
    if ((ty & (2 * st - 1)) == 0) sh[threadIdx.x] += sh[threadIdx.x + st * CX];
    __syncthreads();
  }
  if (ty == 0 && colok) mean[tx] = sh[tx] / sigma;
  if (threadIdx.x == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// k_cert_fin_w's grid, thread-to-element map and grid_reduce order on the centred residual. rh and rc
// may be the same array (an element is read before it is written, by its own thread). The sums:
//   [sum w r_c^2, sum w r_c b, sum v r_c^2 (HOLD: the hold-out loss with the training intercept)]
// with every product formed as in k_cert_fin_w; a zero-weight row is centred like any other.
template <typename T, bool HOLD>
__global__ __launch_bounds__(256) void k_cert_fin_c(const T* rh, const T* __restrict__ b, const T* __restrict__ w,
                                                    const T* __restrict__ hv, const double* __restrict__ mean,
                                                    T* rc, T* __restrict__ rw, int64_t ml, int64_t l, Red red) {
  double v[HOLD ? 3 : 2] = {};
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool narrow = ml <= (int64_t)0xffffffffll;   // uniform: l <= ml
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < ml; idx += stride) {
    const int64_t row = narrow ? (int64_t)((unsigned)idx / (unsigned)l) : idx / l;
    const int64_t col = idx - row * l;
    const T bv = b[idx];
    const T wv = w != nullptr ? w[row] : T(1);
    const T rv = (T)((double)rh[idx] - mean[col]);
    if (rc != nullptr) rc[idx] = rv;
    rw[idx] = wv * rv;
    const double wr = (double)wv * (double)rv;
    v[0] += wr * (double)rv;
    v[1] += wr * (double)bv;
    if constexpr (HOLD) v[2] += ((double)hv[row] * (double)rv) * (double)rv;
  }
  grid_reduce<HOLD ? 3 : 2, 0u>(v, red);
}

// Rows of x are owned by LPR lanes holding EPL elements strided by LPR (kernels_elem.hip's layout)
template <typename T, int LPR, int EPL>
__global__ __launch_bounds__(256) void k_cert_row(const T* __restrict__ x, const T* __restrict__ g, int S,
                                                  T* __restrict__ gout, double* __restrict__ rn, int64_t n,
                                                  int64_t l, double mu_, Red red) {
  const T mu = (T)mu_;
  const int64_t nl = n * l;
  double acc[5] = {0.0, -__builtin_inf(), -__builtin_inf(), 0.0, 0.0};
  const int sub = threadIdx.x & (LPR - 1);
  const int64_t rows_per_block = 256 / LPR;
  const int64_t row_stride = (int64_t)gridDim.x * rows_per_block;
  const int64_t n_trips = (n + row_stride - 1) / row_stride;
  for (int64_t trip = 0; trip < n_trips; ++trip) {   // uniform trip count: every lane shuffles
    const int64_t row = trip * row_stride + (int64_t)blockIdx.x * rows_per_block + (threadIdx.x / LPR);
    const bool rv = row < n;
    const int64_t base = (rv ? row : 0) * l;
    T xv[EPL], gv[EPL];
    bool ok[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPR;
      ok[e] = rv && j < l;
      xv[e] = ok[e] ? x[base + j] : T(0);
      gv[e] = ok[e] ? slab_sum(g, S, nl, base + j) : T(0);
      if (ok[e] && gout != nullptr) gout[base + j] = gv[e];
    }
    const T gn = cert_row<T, LPR, EPL>(xv, gv, ok, rv, sub, mu, acc);
    if (rv && sub == 0 && rn != nullptr) rn[row] = (double)gn;
  }
  grid_reduce<5, 0x6u>(acc, red);
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
template <typename T>
void launch_cert_fin(const T* P, int S, const T* b, T* r, int64_t ml, Red red, hipStream_t st) {
  hipLaunchKernelGGL(k_cert_fin<T>, dim3(cert_grid_for(ml, 256)), dim3(256), 0, st, P, S, b, r, ml, red);
}

template <typename T>
void launch_cert_fin_w(const T* P, int S, const T* b, const T* w, const T* hv, T* r, T* rw, int64_t ml, int64_t l,
                       Red red, hipStream_t st) {
  const dim3 grid(cert_grid_for(ml, 256));   // (k_cert_fin's grid: the same partials, the same order)
  if (hv != nullptr)
    hipLaunchKernelGGL((k_cert_fin_w<T, true>), grid, dim3(256), 0, st, P, S, b, w, hv, r, rw, ml, l, red);
  else
    hipLaunchKernelGGL((k_cert_fin_w<T, false>), grid, dim3(256), 0, st, P, S, b, w, hv, r, rw, ml, l, red);
}

template <typename T>
void launch_cert_csum(const T* P, int S, const T* b, const T* w, T* rh, int64_t m, int64_t l, double sigma,
                      double* part, unsigned* cnt, double* mean, hipStream_t st) {
  if (l < 1 || l > kMaxL) throw Error{GLX_E_INVALID, "the centring finalize takes 1 <= l <= 128"};
  int cx_log = 0;
  while ((int64_t(1) << cx_log) < l) ++cx_log;
  const unsigned grid = cert_grid_for(m, 256 >> cx_log);
  hipLaunchKernelGGL(k_cert_csum<T>, dim3(grid < (unsigned)kCsumBlocks ? grid : (unsigned)kCsumBlocks), dim3(256), 0,
                     st, P, S, b, w, rh, m, l, cx_log, sigma, part, cnt, mean);
}

template <typename T>
void launch_cert_fin_c(const T* rh, const T* b, const T* w, const T* hv, const double* mean, T* rc, T* rw,
                       int64_t ml, int64_t l, Red red, hipStream_t st) {
  const dim3 grid(cert_grid_for(ml, 256));   // (k_cert_fin's grid: the same partials, the same order)
  if (hv != nullptr)
    hipLaunchKernelGGL((k_cert_fin_c<T, true>), grid, dim3(256), 0, st, rh, b, w, hv, mean, rc, rw, ml, l, red);
  else
    hipLaunchKernelGGL((k_cert_fin_c<T, false>), grid, dim3(256), 0, st, rh, b, w, hv, mean, rc, rw, ml, l, red);
}

template <typename T, int LPR, int EPL>
static void cert_row_go(const T* x, const T* g, int S, T* gout, double* rn, int64_t n, int64_t l, double mu,
                        Red red, hipStream_t st) {
  unsigned grid = cert_grid_for(n, 256 / LPR);
  if (grid > 512u) grid = 512u;   // two trips per workgroup at n = 16384 (kernels_elem.hip kRowBlocks)
  hipLaunchKernelGGL((k_cert_row<T, LPR, EPL>), dim3(grid), dim3(256), 0, st, x, g, S, gout, rn, n, l, mu, red);
}
// F receives (lpr_constant, epl_constant): LPR = the power of two >= l up to 16, then EPL up to 8
// at LPR 16 (kernels_elem.hip dispatch_row)
template <typename F>
static void cert_dispatch_row(int64_t l, F&& f) {
#define GLX_CERT_LE(LPR, EPL) f(std::integral_constant<int, LPR>{}, std::integral_constant<int, EPL>{})
  if (l <= 1) GLX_CERT_LE(1, 1);
  else if (l <= 2) GLX_CERT_LE(2, 1);
  else if (l <= 4) GLX_CERT_LE(4, 1);
  else if (l <= 8) GLX_CERT_LE(8, 1);
  else if (l <= 16) GLX_CERT_LE(16, 1);
  else if (l <= 32) GLX_CERT_LE(16, 2);
  else if (l <= 48) GLX_CERT_LE(16, 3);
  else if (l <= 64) GLX_CERT_LE(16, 4);
  else if (l <= 80) GLX_CERT_LE(16, 5);
  else if (l <= 96) GLX_CERT_LE(16, 6);
  else if (l <= 112) GLX_CERT_LE(16, 7);
  else GLX_CERT_LE(16, 8);
#undef GLX_CERT_LE
}
template <typename T>
void launch_cert_row(const T* x, const T* g, int S, T* gout, double* rn, int64_t n, int64_t l, double mu,
                     Red red, hipStream_t st) {
  if (l < 1 || l > kMaxL) throw Error{GLX_E_INVALID, "the certificate's row kernel takes 1 <= l <= 128"};
  cert_dispatch_row(l, [&](auto lpr, auto epl) {
    cert_row_go<T, decltype(lpr)::value, decltype(epl)::value>(x, g, S, gout, rn, n, l, mu, red, st);
  });
}

#define GLX_CERT_INST(T)                                                                              \
  template void launch_cert_fin<T>(const T*, int, const T*, T*, int64_t, Red, hipStream_t);           \
  template void launch_cert_fin_w<T>(const T*, int, const T*, const T*, const T*, T*, T*, int64_t,    \
                                     int64_t, Red, hipStream_t);                                      \
  template void launch_cert_csum<T>(const T*, int, const T*, const T*, T*, int64_t, int64_t, double,  \
                                    double*, unsigned*, double*, hipStream_t);                        \
  template void launch_cert_fin_c<T>(const T*, const T*, const T*, const T*, const double*, T*, T*,   \
                                     int64_t, int64_t, Red, hipStream_t);                             \
  template void launch_cert_row<T>(const T*, const T*, int, T*, double*, int64_t, int64_t, double, Red, \
                                   hipStream_t);

GLX_CERT_INST(double)
GLX_CERT_INST(float)

}  // namespace glx
