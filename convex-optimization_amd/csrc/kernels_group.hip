// kernels_group.hip — the kernels of feature groups and weights (DESIGN.md "Feature groups and
// weights"): the penalty mu sum_g w_g ||x_[g]||_F over contiguous row ranges [ptr[g], ptr[g + 1])
// of the row-major n x l iterate, i.e. over contiguous runs of (ptr[g + 1] - ptr[g]) l elements.
//   k_group_fista   the FISTA step on a given gradient (S slabs of launch_atr): the group prox,
//                   fista_row's momentum arithmetic per element, the four sums
//   k_group_cert    the certificate's group terms on a given g, the five sums, ||g_[g]|| / w_g
//   k_group_cnorm   gcn[g] = sqrt(sum_{i in [g]} cn[i]^2) / w_g in double, and its maximum
//   k_group_expand  kept groups -> kept rows, the reduced ptr / weights / gcn / group map
// Lane layout: a team of LPG adjacent lanes (a power of two up to the wave) owns a run and lane
// `sub` takes its elements sub, sub + LPG, ...; the teams of the grid take the groups in a fixed
// stride, every team the same number of trips. A run of at most LPG EPL elements is read once and
// held in registers; a longer one (the form EPL = 0, a whole wave per run) takes a second sweep
// that re-reads it. Either way a lane adds its elements in ascending order and the team combines
// by an xor butterfly, so every figure is a function of the inputs and the shape alone; the grid
// sums go through grid_reduce. mu, t and the weights are rounded to T first, as in kernels_elem.hip.
#include <cstdlib>
#include <type_traits>

#include "glx.h"
#include "glx_device.h"

namespace glx {

static unsigned group_grid(int64_t G, int lpg) { return (unsigned)clampi(cdiv(G, 256 / lpg), 1, kMaxBlocks); }

// The walk of the teams over the groups: `grp` is this team's group of the trip (>= G: none).
#define GLX_GROUP_LOOP_BEGIN(LPG)                                                          \
  const int sub = threadIdx.x & ((LPG)-1);                                                 \
  const int64_t teams_ = 256 / (LPG);                                                      \
  const int64_t gstride_ = (int64_t)gridDim.x * teams_;                                    \
  const int64_t trips_ = (G + gstride_ - 1) / gstride_;                                    \
  for (int64_t trip_ = 0; trip_ < trips_; ++trip_) {   /* uniform: every lane shuffles */  \
    const int64_t grp = trip_ * gstride_ + (int64_t)blockIdx.x * teams_ + (threadIdx.x / (LPG));
#define GLX_GROUP_LOOP_END }

template <typename T, int LPG, int EPL>
__global__ __launch_bounds__(256) void k_group_fista(const T* __restrict__ y, const T* __restrict__ g, int S,
                                                     const T* __restrict__ xk, T* __restrict__ xc,
                                                     T* __restrict__ vnext, T* __restrict__ ynext,
                                                     const int* __restrict__ ptr, const double* __restrict__ wts,
                                                     int64_t G, int64_t nrows, int64_t l, double t_, double tmu_,
                                                     double thres_, double theta_, double a1_, double b1_, Red red) {
  static_assert(EPL > 0 || LPG == 64, "the two-sweep form gives a run a whole wave");
  const T t = (T)t_, tmu = (T)tmu_, thres = (T)thres_, theta = (T)theta_, a1 = (T)a1_, b1 = (T)b1_;
  const int64_t nl = nrows * l;
  double acc[4] = {0.0, 0.0, 0.0, -__builtin_inf()};
  GLX_GROUP_LOOP_BEGIN(LPG)
  const GroupRun<T> run = group_run<T>(ptr, wts, grp, G, l);
  const T tmuw = tmu * run.w;   // t mu w_g, once per group
  T psq = T(0);
  if constexpr (EPL > 0) {
    T yv[EPL], gv[EPL], w[EPL];
    bool ok[EPL];
    T sq = T(0);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPG;
      ok[e] = j < run.len;
      yv[e] = ok[e] ? y[run.base + j] : T(0);
      gv[e] = ok[e] ? slab_sum(g, S, nl, run.base + j) : T(0);
      w[e] = yv[e] - t * gv[e];
      sq = sq + w[e] * w[e];
    }
    const T nrm = __builtin_sqrt(row_allsum<LPG>(sq));
    T c = nrm - tmuw;
    c = (c < T(0)) ? T(0) : c;   // NaN compares false and stays
    const T d = ((nrm < thres) ? T(1) : T(0)) + nrm;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPG;
      const T xo = ok[e] ? xk[run.base + j] : T(0);
      const T pv = (w[e] * c) / d;
      T vn, yn;
      fista_elem<T>(pv, yv[e], gv[e], xo, ok[e], thres, theta, a1, b1, vn, yn, acc, psq);
      if (ok[e]) {
        xc[run.base + j] = pv;
        vnext[run.base + j] = vn;
        ynext[run.base + j] = yn;
      }
    }
  } else {
    T sq = T(0);
#pragma unroll 4
    for (int64_t j = sub; j < run.len; j += LPG) {
      const T wv = y[run.base + j] - t * slab_sum(g, S, nl, run.base + j);
      sq = sq + wv * wv;
    }
    const T nrm = __builtin_sqrt(row_allsum<LPG>(sq));
    T c = nrm - tmuw;
    c = (c < T(0)) ? T(0) : c;
    const T d = ((nrm < thres) ? T(1) : T(0)) + nrm;
#pragma unroll 4
    for (int64_t j = sub; j < run.len; j += LPG) {   // the second sweep: the run is in L2
      const T yv = y[run.base + j];
      const T gv = slab_sum(g, S, nl, run.base + j);
      const T wv = yv - t * gv;
      const T pv = (wv * c) / d;
      T vn, yn;
      fista_elem<T>(pv, yv, gv, xk[run.base + j], true, thres, theta, a1, b1, vn, yn, acc, psq);
      xc[run.base + j] = pv;
      vnext[run.base + j] = vn;
      ynext[run.base + j] = yn;
    }
  }
  const T ps = row_allsum<LPG>(psq);
  if (run.ok && sub == 0) acc[2] += (double)(run.w * __builtin_sqrt(ps));
  GLX_GROUP_LOOP_END
  // rows from ptr[G] up to the padded width belong to no group
  for (int64_t idx = (int64_t)ptr[G] * l + (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nl;
       idx += (int64_t)gridDim.x * 256) {
    xc[idx] = T(0);
    vnext[idx] = T(0);
    ynext[idx] = T(0);
  }
  grid_reduce<4, 0x8u>(acc, red);
}

template <typename T, int LPG, int EPL>
__global__ __launch_bounds__(256) void k_group_cert(const T* __restrict__ x, const T* __restrict__ g, int S,
                                                    T* __restrict__ gout, double* __restrict__ rn,
                                                    const int* __restrict__ ptr, const double* __restrict__ wts,
                                                    int64_t G, int64_t nrows, int64_t l, double mu_, Red red) {
  static_assert(EPL > 0 || LPG == 64, "the two-sweep form gives a run a whole wave");
  const T mu = (T)mu_;
  const int64_t nl = nrows * l;
  double acc[5] = {0.0, -__builtin_inf(), -__builtin_inf(), 0.0, 0.0};
  GLX_GROUP_LOOP_BEGIN(LPG)
  const GroupRun<T> run = group_run<T>(ptr, wts, grp, G, l);
  const T muw = mu * run.w;   // mu w_g, once per group
  T gn, xn, kn;
  if constexpr (EPL > 0) {
    T xv[EPL], gv[EPL];
    bool ok[EPL];
    T gsq = T(0), xsq = T(0);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int64_t j = sub + (int64_t)e * LPG;
      ok[e] = j < run.len;
      xv[e] = ok[e] ? x[run.base + j] : T(0);
      gv[e] = ok[e] ? slab_sum(g, S, nl, run.base + j) : T(0);
      if (ok[e] && gout != nullptr) gout[run.base + j] = gv[e];
      if (ok[e]) {
        gsq = gsq + gv[e] * gv[e];
        xsq = xsq + xv[e] * xv[e];
      }
    }
    gn = __builtin_sqrt(row_allsum<LPG>(gsq));
    xn = __builtin_sqrt(row_allsum<LPG>(xsq));
    T ksq = T(0);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const T k = gv[e] + (muw * xv[e]) / xn;   // (0 / 0 in a zero group: not selected)
      if (ok[e]) ksq = ksq + k * k;
    }
    kn = __builtin_sqrt(row_allsum<LPG>(ksq));
  } else {
    T gsq = T(0), xsq = T(0);
#pragma unroll 4
    for (int64_t j = sub; j < run.len; j += LPG) {
      const T xv = x[run.base + j];
      const T gv = slab_sum(g, S, nl, run.base + j);
      if (gout != nullptr) gout[run.base + j] = gv;
      gsq = gsq + gv * gv;
      xsq = xsq + xv * xv;
    }
    gn = __builtin_sqrt(row_allsum<LPG>(gsq));
    xn = __builtin_sqrt(row_allsum<LPG>(xsq));
    T ksq = T(0);
#pragma unroll 4
    for (int64_t j = sub; j < run.len; j += LPG) {   // the second sweep: the run is in L2
      const T k = slab_sum(g, S, nl, run.base + j) + (muw * x[run.base + j]) / xn;
      ksq = ksq + k * k;
    }
    kn = __builtin_sqrt(row_allsum<LPG>(ksq));
  }
  const T gq = group_cert_terms<T>(gn, xn, kn, muw, run.w, run.ok && sub == 0, acc);
  if (run.ok && sub == 0 && rn != nullptr) rn[grp] = (double)gq;
  GLX_GROUP_LOOP_END
  if (gout != nullptr)   // rows that belong to no group: g all the same
    for (int64_t idx = (int64_t)ptr[G] * l + (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nl;
         idx += (int64_t)gridDim.x * 256)
      gout[idx] = slab_sum(g, S, nl, idx);
  grid_reduce<5, 0x6u>(acc, red);
}

// gcn[g] = sqrt(sum_{i in [g]} cn[i]^2) / w_g in double; red.out = [max_g gcn[g]] (NaN-propagating)
template <int LPG>
__global__ __launch_bounds__(256) void k_group_cnorm(const double* __restrict__ cn, const int* __restrict__ ptr,
                                                     const double* __restrict__ wts, int64_t G,
                                                     double* __restrict__ gcn, Red red) {
  double acc[1] = {-__builtin_inf()};
  GLX_GROUP_LOOP_BEGIN(LPG)
  const bool ok = grp < G;
  const int64_t r0 = ok ? ptr[grp] : 0, r1 = ok ? ptr[grp + 1] : 0;
  double sq = 0.0;
  for (int64_t i = r0 + sub; i < r1; i += LPG) {
    const double c = cn[i];
    sq += c * c;
  }
  sq = row_allsum<LPG>(sq);
  if (ok && sub == 0) {
    const double v = __builtin_sqrt(sq) / wts[grp];
    gcn[grp] = v;
    acc[0] = nan_max(acc[0], v);
  }
  GLX_GROUP_LOOP_END
  grid_reduce<1, 0x1u>(acc, red);
}

// One workgroup. klist: kcnt[0] = K kept groups of the current problem, ascending. Thread t owns a
// contiguous chunk of the list; the chunks' row counts are scanned in thread order (k_screen's
// scan), and every thread writes its groups' reduced offsets, weights, gcn and full-problem ids and
// their rows, ascending from the group's offset. The loads of a chunk are independent of each other
// (the loops are unrolled so that several are in flight) and the stores wait for nothing. A group of
// more than kExpandLong rows is left to the whole workgroup instead: its list index and offset go
// to an LDS list (the slot order is whatever it is; every entry names its own destination, so the
// output does not depend on it) and all threads fill its rows after a barrier; a group that finds
// the list full is written by its own thread. Integers only and no atomics on data: the same output
// every run.
//   rows_out: the kept rows of the current problem, ascending, then -1 up to ecnt[1];
//   ptr_out (K + 1), w_out, gcn_out, map_out (K): the reduced problem's; map_out names groups of
//   the full problem (map == NULL: the current problem is the full one);  ecnt = [rows, rows
//   rounded up to 64].
constexpr int kExpandLong = 256;
constexpr int kExpandLongCap = 512;
__global__ __launch_bounds__(256) void k_group_expand(const int* __restrict__ klist, const int* __restrict__ kcnt,
                                                      const int* __restrict__ ptr, const double* __restrict__ wts,
                                                      const double* __restrict__ gcn, const int* __restrict__ map,
                                                      int* __restrict__ rows_out, int* __restrict__ ptr_out,
                                                      double* __restrict__ w_out, double* __restrict__ gcn_out,
                                                      int* __restrict__ map_out, int* __restrict__ ecnt) {
  __shared__ long long offs[257];
  __shared__ int long_r0[kExpandLongCap], long_run[kExpandLongCap], long_off[kExpandLongCap];
  __shared__ int nlong;
  if (threadIdx.x == 0) nlong = 0;
  const int64_t K = kcnt[0];
  const int64_t C = (K + 255) / 256;
  const int64_t k0 = (int64_t)threadIdx.x * C < K ? (int64_t)threadIdx.x * C : K;
  const int64_t k1 = k0 + C < K ? k0 + C : K;
  long long c = 0;
#pragma unroll 8
  for (int64_t k = k0; k < k1; ++k) {
    const int gi = klist[k];
    c += ptr[gi + 1] - ptr[gi];
  }
  offs[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {   // 256 chunk offsets, in thread order
    long long run = 0;
    for (int t = 0; t < 256; ++t) {
      const long long v = offs[t];
      offs[t] = run;
      run += v;
    }
    offs[256] = run;
  }
  __syncthreads();
  long long o = offs[threadIdx.x];
#pragma unroll 4
  for (int64_t k = k0; k < k1; ++k) {
    const int gi = klist[k];
    const int r0 = ptr[gi], run = ptr[gi + 1] - r0;
    ptr_out[k] = (int)o;
    w_out[k] = wts[gi];
    gcn_out[k] = gcn[gi];
    map_out[k] = map != nullptr ? map[gi] : gi;
    bool mine = true;
    if (run > kExpandLong) {
      const int slot = atomicAdd(&nlong, 1);
      if (slot < kExpandLongCap) {
        long_r0[slot] = r0;
        long_run[slot] = run;
        long_off[slot] = (int)o;
        mine = false;
      }
    }
    if (mine)
      for (int j = 0; j < run; ++j) rows_out[o + j] = r0 + j;
    o += run;
  }
  const long long total = offs[256];
  if (threadIdx.x == 0) ptr_out[K] = (int)total;
  __syncthreads();
  const int nl = nlong < kExpandLongCap ? nlong : kExpandLongCap;
  for (int q = 0; q < nl; ++q) {
    const int r0 = long_r0[q], run = long_run[q];
    int* dst = rows_out + long_off[q];
    for (int j = threadIdx.x; j < run; j += 256) dst[j] = r0 + j;
  }
  const long long wp = (total + 63) / 64 * 64;
  for (long long q = total + threadIdx.x; q < wp; q += 256) rows_out[q] = -1;
  if (threadIdx.x == 0) {
    ecnt[0] = (int)total;
    ecnt[1] = (int)wp;
  }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
// F receives (lpg_constant, epl_constant) for the longest run of the problem, max_len elements:
// the smallest team that holds it with one element per lane, then up to 8 elements per lane of a
// whole wave, then the two-sweep form (EPL 0), which takes any length.
template <typename F>
static void group_dispatch(int64_t max_len, F&& f) {
#define GLX_GROUP_LE(LPG, EPL) f(std::integral_constant<int, LPG>{}, std::integral_constant<int, EPL>{})
  if (max_len <= 4) GLX_GROUP_LE(4, 1);
  else if (max_len <= 16) GLX_GROUP_LE(16, 1);
  else if (max_len <= 32) GLX_GROUP_LE(32, 1);
  else if (max_len <= 64) GLX_GROUP_LE(64, 1);
  else if (max_len <= 128) GLX_GROUP_LE(64, 2);
  else if (max_len <= 256) GLX_GROUP_LE(64, 4);
  else if (max_len <= 512) GLX_GROUP_LE(64, 8);
  else GLX_GROUP_LE(64, 0);
#undef GLX_GROUP_LE
}
std::string group_layout(int64_t max_len) {
  std::string s;
  group_dispatch(max_len, [&](auto lpg, auto epl) {
    const int L = decltype(lpg)::value, E = decltype(epl)::value;
    s = std::to_string(L) + " lanes per group, " +
        (E > 0 ? std::to_string(E) + " element(s) per lane in registers" : std::string("two sweeps"));
  });
  return s;
}

static void group_check(int64_t G, int64_t nrows, int64_t l, int64_t max_run) {
  if (G < 1 || nrows < 1 || max_run < 1) throw Error{GLX_E_INVALID, "group kernels: G, rows and max_run must be positive"};
  if (l < 1 || l > kMaxL) throw Error{GLX_E_INVALID, "the group kernels take 1 <= l <= 128"};
}

template <typename T>
void launch_group_fista(const T* y, const T* g, int S, const T* xk, T* xc, T* vnext, T* ynext, const int* ptr,
                        const double* wts, int64_t G, int64_t nrows, int64_t l, int64_t max_run, double t, double mu,
                        double thres, double theta, double theta_next, Red red, hipStream_t st) {
  group_check(G, nrows, l, max_run);
  group_dispatch(max_run * l, [&](auto lpg, auto epl) {
    constexpr int L = decltype(lpg)::value, E = decltype(epl)::value;
    hipLaunchKernelGGL((k_group_fista<T, L, E>), dim3(group_grid(G, L)), dim3(256), 0, st, y, g, S, xk, xc, vnext,
                       ynext, ptr, wts, G, nrows, l, t, t * mu, thres, theta, 1.0 - theta_next, theta_next, red);
  });
}

template <typename T>
void launch_group_cert(const T* x, const T* g, int S, T* gout, double* rn, const int* ptr, const double* wts,
                       int64_t G, int64_t nrows, int64_t l, int64_t max_run, double mu, Red red, hipStream_t st) {
  group_check(G, nrows, l, max_run);
  group_dispatch(max_run * l, [&](auto lpg, auto epl) {
    constexpr int L = decltype(lpg)::value, E = decltype(epl)::value;
    hipLaunchKernelGGL((k_group_cert<T, L, E>), dim3(group_grid(G, L)), dim3(256), 0, st, x, g, S, gout, rn, ptr, wts,
                       G, nrows, l, mu, red);
  });
}

void launch_group_cnorm(const double* cn, const int* ptr, const double* wts, int64_t G, int64_t max_run, double* gcn,
                        Red red, hipStream_t st) {
  if (G < 1) throw Error{GLX_E_INVALID, "group kernels: G must be positive"};
  if (max_run <= 8)   // a lane per group; longer runs a wave each
    hipLaunchKernelGGL(k_group_cnorm<1>, dim3(group_grid(G, 1)), dim3(256), 0, st, cn, ptr, wts, G, gcn, red);
  else
    hipLaunchKernelGGL(k_group_cnorm<64>, dim3(group_grid(G, 64)), dim3(256), 0, st, cn, ptr, wts, G, gcn, red);
}

void launch_group_expand(const int* klist, const int* kcnt, const int* ptr, const double* wts, const double* gcn,
                         const int* map, int* rows_out, int* ptr_out, double* w_out, double* gcn_out, int* map_out,
                         int* ecnt, hipStream_t st) {
  hipLaunchKernelGGL(k_group_expand, dim3(1), dim3(256), 0, st, klist, kcnt, ptr, wts, gcn, map, rows_out, ptr_out,
                     w_out, gcn_out, map_out, ecnt);
}

#define GLX_GROUP_INST(T)                                                                                        \
  template void launch_group_fista<T>(const T*, const T*, int, const T*, T*, T*, T*, const int*, const double*,   \
                                      int64_t, int64_t, int64_t, int64_t, double, double, double, double, double, \
                                      Red, hipStream_t);                                                          \
  template void launch_group_cert<T>(const T*, const T*, int, T*, double*, const int*, const double*, int64_t,    \
                                     int64_t, int64_t, int64_t, double, Red, hipStream_t);

GLX_GROUP_INST(double)
GLX_GROUP_INST(float)

}  // namespace glx
