// kernels_sgl.hip — the kernels of the sparse-group lasso (DESIGN.md "Sparse-group lasso"): the penalty
//   mu Omega_tau(x) = a sum_i ||x_i||_2 + sum_g c_g ||x_[g]||_F,   a = tau mu,  c_g = (1 - tau) mu w_g,
// over the contiguous row ranges [ptr[g], ptr[g + 1]) of the row-major n x l iterate.
//   k_sgl_fista       the FISTA step on a given gradient (S slabs of launch_atr): the two-level prox,
//                     fista_elem's momentum per element, the four sums
//   k_sgl_cert        the certificate's terms on a given g: the row norms rho_i = ||g_i||, the KKT
//                     distances, Omega_tau(x), six sums
//   k_sgl_dual_scale  s_g = sup{s : phi_g(s) <= c_g}, phi_g(s) = sqrt(sum_{i in g} (s rho_i - a)_+^2), on
//                     the n row norms, by a fixed number of halvings; two solves a launch
//   k_sgl_screen      the row and the group test of gap-safe screening: a kept flag per row
//   k_sgl_expand      kept rows -> the ascending row list and the reduced ptr / weights / gcn / map
// Lane layout of the first two: a wave owns a group, a sub-team of LPR adjacent lanes (a power of two,
// >= l up to the wave) owns a row, lane `c` of it the columns c, c + LPR (RE = 2 of them for l > 64),
// and the 64 / LPR sub-teams take the group's rows in a fixed stride, every sub-team the same number
// of trips. A lane adds its elements in ascending order, the sub-team combines by an xor butterfly
// (a row's sum), a sub-team adds its rows' figures in ascending order and the sub-teams combine by the
// butterfly's remaining steps (a group's sum): every figure is a function of the inputs and the shape
// alone. The second sweep over a group re-reads it (it is in L2). The grid sums go through
// grid_reduce; mu, t, tau and the weights are rounded to T first, as in kernels_group.hip. The last
// three kernels work in double on n doubles. No atomics on data anywhere.
#include <cstdlib>
#include <type_traits>

#include "glx.h"
#include "glx_device.h"

namespace glx {

static unsigned sgl_grid(int64_t G) { return (unsigned)clampi(cdiv(G, 4), 1, kMaxBlocks); }

// The walk of the waves over the groups: `grp` is this wave's group of the trip (>= G: none).
#define GLX_SGL_LOOP_BEGIN                                                                 \
  const int sub = threadIdx.x & 63;                                                        \
  const int64_t gstride_ = (int64_t)gridDim.x * 4;                                         \
  const int64_t trips_ = (G + gstride_ - 1) / gstride_;                                    \
  for (int64_t trip_ = 0; trip_ < trips_; ++trip_) {   /* uniform: every lane shuffles */  \
    const int64_t grp = trip_ * gstride_ + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   \
    const bool gok = grp < G;                                                              \
    const int64_t r0 = gok ? ptr[grp] : 0, r1 = gok ? ptr[grp + 1] : 0;
#define GLX_SGL_LOOP_END }

// the butterfly's steps across the sub-teams of a wave (every lane of a sub-team holds the same v)
template <int LPR, typename T>
__device__ inline T sgl_teamsum(T v) {
#pragma unroll
  for (int off = 32; off >= LPR; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ inline double sgl_wavemax(double v) {   // NaN-propagating
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = nan_max(v, __shfl_xor(v, off));
  return v;
}

template <typename T, int LPR, int RE>
__global__ __launch_bounds__(256) void k_sgl_fista(const T* __restrict__ y, const T* __restrict__ g, int S,
                                                   const T* __restrict__ xk, T* __restrict__ xc,
                                                   T* __restrict__ vnext, T* __restrict__ ynext,
                                                   const int* __restrict__ ptr, const double* __restrict__ wts,
                                                   int64_t G, int64_t nrows, int64_t l, double t_, double ta_,
                                                   double tc_, double tau_, double omt_, double thres_,
                                                   double theta_, double a1_, double b1_, Red red) {
  constexpr int NST = 64 / LPR;
  const T t = (T)t_, ta = (T)ta_, tc = (T)tc_, tau = (T)tau_, omt = (T)omt_, thres = (T)thres_, theta = (T)theta_,
          a1 = (T)a1_, b1 = (T)b1_;
  const int64_t nl = nrows * l;
  double acc[4] = {0.0, 0.0, 0.0, -__builtin_inf()};
  GLX_SGL_LOOP_BEGIN
  const int c = sub & (LPR - 1), st = sub / LPR;
  const T wg = gok ? (T)wts[grp] : T(1);
  const T tcw = tc * wg;   // t (1 - tau) mu w_g, once per group
  const int64_t rtrips = (r1 - r0 + NST - 1) / NST;   // uniform over the wave
  // first sweep: q_g^2 = sum_i (rho_i - t a)_+^2
  T qsq = T(0);
  for (int64_t k = 0; k < rtrips; ++k) {
    const int64_t i = r0 + st + k * NST;
    const bool rok = i < r1;
    T sq = T(0);
#pragma unroll
    for (int e = 0; e < RE; ++e) {
      const int64_t col = c + e * LPR;
      const bool ok = rok && col < l;
      const int64_t idx = i * l + col;
      const T wv = ok ? y[idx] - t * slab_sum(g, S, nl, idx) : T(0);
      sq = sq + wv * wv;
    }
    const T rho = __builtin_sqrt(row_allsum<LPR>(sq));
    T c1 = rho - ta;
    c1 = (c1 < T(0)) ? T(0) : c1;   // NaN compares false and stays
    if (rok) qsq = qsq + c1 * c1;
  }
  const T q = __builtin_sqrt(sgl_teamsum<LPR>(qsq));
  T c2 = q - tcw;
  c2 = (c2 < T(0)) ? T(0) : c2;
  const T d2 = ((q < thres) ? T(1) : T(0)) + q;
  // second sweep: the run is in L2
  T gpsq = T(0);
  for (int64_t k = 0; k < rtrips; ++k) {
    const int64_t i = r0 + st + k * NST;
    const bool rok = i < r1;
    T yv[RE], gv[RE], wv[RE];
    bool ok[RE];
    T sq = T(0);
#pragma unroll
    for (int e = 0; e < RE; ++e) {
      const int64_t col = c + e * LPR;
      ok[e] = rok && col < l;
      const int64_t idx = i * l + col;
      yv[e] = ok[e] ? y[idx] : T(0);
      gv[e] = ok[e] ? slab_sum(g, S, nl, idx) : T(0);
      wv[e] = yv[e] - t * gv[e];
      sq = sq + wv[e] * wv[e];
    }
    const T rho = __builtin_sqrt(row_allsum<LPR>(sq));
    T c1 = rho - ta;
    c1 = (c1 < T(0)) ? T(0) : c1;
    const T d1 = ((rho < thres) ? T(1) : T(0)) + rho;
    const bool zero = c1 == T(0) || c2 == T(0);   // (a NaN is neither: it stays)
    T psq = T(0);
#pragma unroll
    for (int e = 0; e < RE; ++e) {
      const int64_t idx = i * l + c + e * LPR;
      const T xo = ok[e] ? xk[idx] : T(0);
      const T uv = (wv[e] * c1) / d1;
      const T pv = zero ? T(0) : (uv * c2) / d2;   // a zero row or group is +0
      T vn, yn;
      fista_elem<T>(pv, yv[e], gv[e], xo, ok[e], thres, theta, a1, b1, vn, yn, acc, psq);
      if (ok[e]) {
        xc[idx] = pv;
        vnext[idx] = vn;
        ynext[idx] = yn;
      }
    }
    const T ps = row_allsum<LPR>(psq);
    if (rok) gpsq = gpsq + ps;
    if (rok && c == 0) acc[2] += (double)(tau * __builtin_sqrt(ps));
  }
  const T gps = sgl_teamsum<LPR>(gpsq);
  if (gok && sub == 0) acc[2] += (double)(omt * (wg * __builtin_sqrt(gps)));
  GLX_SGL_LOOP_END
  // rows from ptr[G] up to the padded width belong to no group
  for (int64_t idx = (int64_t)ptr[G] * l + (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nl;
       idx += (int64_t)gridDim.x * 256) {
    xc[idx] = T(0);
    vnext[idx] = T(0);
    ynext[idx] = T(0);
  }
  grid_reduce<4, 0x8u>(acc, red);
}

// red.out = [Omega_tau(x), max_i rho_i, max kkt, sum kkt^2, nonzero groups, nonzero rows]; rn (may be
// NULL) receives rho_i = ||g_i|| as nrows-independent n doubles, gout (may be NULL) g. The KKT distance
// from -g to mu dOmega_tau(x): a nonzero row of a nonzero group ||g_i + a x_i / ||x_i|| + c_g x_i /
// ||x_[g]|| ||, a zero row of a nonzero group (rho_i - a)_+, a zero group (phi_g(1) - c_g)_+ (one term).
template <typename T, int LPR, int RE>
__global__ __launch_bounds__(256) void k_sgl_cert(const T* __restrict__ x, const T* __restrict__ g, int S,
                                                  T* __restrict__ gout, double* __restrict__ rn,
                                                  const int* __restrict__ ptr, const double* __restrict__ wts,
                                                  int64_t G, int64_t nrows, int64_t l, double a_, double cb_,
                                                  double tau_, double omt_, Red red) {
  constexpr int NST = 64 / LPR;
  const T a = (T)a_, cb = (T)cb_, tau = (T)tau_, omt = (T)omt_;
  const int64_t nl = nrows * l;
  double acc[6] = {0.0, -__builtin_inf(), -__builtin_inf(), 0.0, 0.0, 0.0};
  GLX_SGL_LOOP_BEGIN
  const int c = sub & (LPR - 1), st = sub / LPR;
  const T wg = gok ? (T)wts[grp] : T(1);
  const T cg = cb * wg;   // (1 - tau) mu w_g, once per group
  const int64_t rtrips = (r1 - r0 + NST - 1) / NST;
  T gxsq = T(0), phsq = T(0);
  for (int64_t k = 0; k < rtrips; ++k) {
    const int64_t i = r0 + st + k * NST;
    const bool rok = i < r1;
    T gsq = T(0), xsq = T(0);
#pragma unroll
    for (int e = 0; e < RE; ++e) {
      const int64_t col = c + e * LPR;
      const bool ok = rok && col < l;
      const int64_t idx = i * l + col;
      const T xv = ok ? x[idx] : T(0);
      const T gv = ok ? slab_sum(g, S, nl, idx) : T(0);
      if (ok && gout != nullptr) gout[idx] = gv;
      gsq = gsq + gv * gv;
      xsq = xsq + xv * xv;
    }
    const T rho = __builtin_sqrt(row_allsum<LPR>(gsq));
    const T xs = row_allsum<LPR>(xsq);
    const T xn = __builtin_sqrt(xs);
    T d = rho - a;
    d = (d < T(0)) ? T(0) : d;   // NaN compares false and stays
    if (rok) {
      gxsq = gxsq + xs;
      phsq = phsq + d * d;
    }
    if (rok && c == 0) {
      if (rn != nullptr) rn[i] = (double)rho;
      acc[0] += (double)(tau * xn);
      acc[1] = nan_max(acc[1], (double)rho);
      acc[5] += (xn != xn) ? (double)xn : (xn != T(0) ? 1.0 : 0.0);
    }
  }
  const T xg = __builtin_sqrt(sgl_teamsum<LPR>(gxsq));
  const T ph = __builtin_sqrt(sgl_teamsum<LPR>(phsq));
  if (gok && sub == 0) {
    acc[0] += (double)(omt * (wg * xg));
    acc[4] += (xg != xg) ? (double)xg : (xg != T(0) ? 1.0 : 0.0);
    if (xg == T(0)) {   // a zero group: one term
      T d = ph - cg;
      d = (d < T(0)) ? T(0) : d;
      acc[2] = nan_max(acc[2], (double)d);
      acc[3] += (double)d * (double)d;
    }
  }
  // second sweep (the run is in L2): the rows of a nonzero group; uniform over the wave
  if (!(xg == T(0))) {
    for (int64_t k = 0; k < rtrips; ++k) {
      const int64_t i = r0 + st + k * NST;
      const bool rok = i < r1;
      T xv[RE], gv[RE];
      T gsq = T(0), xsq = T(0);
#pragma unroll
      for (int e = 0; e < RE; ++e) {
        const int64_t col = c + e * LPR;
        const bool ok = rok && col < l;
        const int64_t idx = i * l + col;
        xv[e] = ok ? x[idx] : T(0);
        gv[e] = ok ? slab_sum(g, S, nl, idx) : T(0);
        gsq = gsq + gv[e] * gv[e];
        xsq = xsq + xv[e] * xv[e];
      }
      const T rho = __builtin_sqrt(row_allsum<LPR>(gsq));
      const T xn = __builtin_sqrt(row_allsum<LPR>(xsq));
      T ksq = T(0);
#pragma unroll
      for (int e = 0; e < RE; ++e) {
        const T kv = (gv[e] + (a * xv[e]) / xn) + (cg * xv[e]) / xg;   // (0 / 0 in a zero row: not selected)
        ksq = ksq + kv * kv;
      }
      const T kn = __builtin_sqrt(row_allsum<LPR>(ksq));
      T d = rho - a;
      d = (d < T(0)) ? T(0) : d;
      const T kkt = (xn == T(0)) ? d : kn;
      if (rok && c == 0) {
        acc[2] = nan_max(acc[2], (double)kkt);
        acc[3] += (double)kkt * (double)kkt;
      }
    }
  }
  GLX_SGL_LOOP_END
  if (gout != nullptr)   // rows that belong to no group: g all the same
    for (int64_t idx = (int64_t)ptr[G] * l + (int64_t)blockIdx.x * 256 + threadIdx.x; idx < nl;
         idx += (int64_t)gridDim.x * 256)
      gout[idx] = slab_sum(g, S, nl, idx);
  grid_reduce<6, 0x6u>(acc, red);
}

// phi_g(s) <= c_g on the padded row norms p_i = mul rho_i + add, evaluated by the whole wave: lane
// `sub` adds its rows r0 + sub, r0 + sub + 64, ... in ascending order, the wave combines by butterfly.
// p0 is the lane's first row's p (0 where it has none), the others are re-read.
__device__ inline bool sgl_feasible(double s, double p0, const double* __restrict__ rho, int64_t r0, int64_t r1,
                                    int sub, double mul, double add, double a, double cg) {
  double v = s * p0 - a;
  v = (v < 0.0) ? 0.0 : v;   // NaN compares false and stays (and then nothing is feasible)
  double sq = (r0 + sub < r1) ? v * v : 0.0;
  for (int64_t i = r0 + sub + 64; i < r1; i += 64) {
    double w = s * (mul * rho[i] + add) - a;
    w = (w < 0.0) ? 0.0 : w;
    sq += w * w;
  }
  sq = row_allsum<64>(sq);
  return __builtin_sqrt(sq) <= cg;
}

// Two solves a launch, q = 0, 1, on p_i = mul[q] rho_i + add[q] sc with sc = sqrt(*rr) (rr NULL: 1):
// sg[q * G + g] (sg may be NULL) = the unclamped s_g, red.out[q] = max_g (-s_g) (NaN-propagating).
// The bracket is [0, hi], hi = (a + c_g) / max_i p_i, where phi_g(hi) >= c_g: hi itself is tried
// first, then kSglHalvings halvings keep the feasible end, which is returned. c_g = 0 (tau = 1):
// a / max_i p_i. A group whose p are all 0: +inf.
constexpr int kSglHalvings = 56;
__global__ __launch_bounds__(256) void k_sgl_dual_scale(const double* __restrict__ rho, const int* __restrict__ ptr,
                                                        const double* __restrict__ wts, int64_t G, double a,
                                                        double cb, double mul0, double add0, double mul1,
                                                        double add1, const double* __restrict__ rr,
                                                        double* __restrict__ sg, Red red) {
  double acc[2] = {-__builtin_inf(), -__builtin_inf()};
  const double sc = rr != nullptr ? __builtin_sqrt(*rr) : 1.0;
  GLX_SGL_LOOP_BEGIN
  const double cg = cb * (gok ? wts[grp] : 1.0);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const double mul = q == 0 ? mul0 : mul1, add = (q == 0 ? add0 : add1) * sc;
    const double p0 = (r0 + sub < r1) ? mul * rho[r0 + sub] + add : 0.0;
    double pm = (r0 + sub < r1) ? p0 : -__builtin_inf();
    for (int64_t i = r0 + sub + 64; i < r1; i += 64) pm = nan_max(pm, mul * rho[i] + add);
    pm = sgl_wavemax(pm);
    double hi = (a + cg) / pm, lo = 0.0;
    if (sgl_feasible(hi, p0, rho, r0, r1, sub, mul, add, a, cg)) lo = hi;
    for (int h = 0; h < kSglHalvings; ++h) {   // the same count for every wave
      const double mid = lo + (hi - lo) * 0.5;
      const bool f = sgl_feasible(mid, p0, rho, r0, r1, sub, mul, add, a, cg);
      lo = f ? mid : lo;
      hi = f ? hi : mid;
    }
    double s = cg == 0.0 ? a / pm : lo;
    if (pm == 0.0) s = __builtin_inf();
    if (pm != pm) s = pm;
    if (gok && sub == 0) {
      if (sg != nullptr) sg[(int64_t)q * G + grp] = s;
      acc[q] = nan_max(acc[q], -s);
    }
  }
  GLX_SGL_LOOP_END
  grid_reduce<2, 0x3u>(acc, red);
}

// keep[i] = 1 where row i is not proven zero: its group's test fails (or group_test == 0) and its own
// does; p_i = mul rho_i + add sqrt(*rr) (rr NULL: add). A NaN anywhere keeps. gkeep (may be NULL): 1 where
// the group keeps at least one row. red.out = [kept groups, kept rows] (exact in double).
//   row:    s p_i + cn_i rad < a_lo
//   group:  sqrt(sum_i (s p_i - a_lo)_+^2) / w_g + gcn_g rad < cb_lo
__global__ __launch_bounds__(256) void k_sgl_screen(const double* __restrict__ rho, const double* __restrict__ cn,
                                                    const double* __restrict__ gcn, const int* __restrict__ ptr,
                                                    const double* __restrict__ wts, int64_t G, double s, double mul,
                                                    double add_, const double* __restrict__ rr, double rad,
                                                    double a_lo, double cb_lo, int group_test,
                                                    int* __restrict__ keep, int* __restrict__ gkeep, Red red) {
  double acc[2] = {0.0, 0.0};
  const double add = add_ * (rr != nullptr ? __builtin_sqrt(*rr) : 1.0);
  GLX_SGL_LOOP_BEGIN
  double sq = 0.0;
  for (int64_t i = r0 + sub; i < r1; i += 64) {
    double v = s * (mul * rho[i] + add) - a_lo;
    v = (v < 0.0) ? 0.0 : v;
    sq += v * v;
  }
  sq = row_allsum<64>(sq);
  const double wg = gok ? wts[grp] : 1.0, gc = gok ? gcn[grp] : 0.0;
  const bool gone = group_test != 0 && (__builtin_sqrt(sq) / wg + gc * rad < cb_lo);   // NaN: kept
  double any = 0.0;
  for (int64_t i = r0 + sub; i < r1; i += 64) {
    const bool rgone = s * (mul * rho[i] + add) + cn[i] * rad < a_lo;
    const int kp = (!gone && !rgone) ? 1 : 0;
    keep[i] = kp;
    any += (double)kp;
  }
  acc[1] += any;
  any = row_allsum<64>(any);
  if (gok && sub == 0) {
    if (gkeep != nullptr) gkeep[grp] = any > 0.0 ? 1 : 0;
    acc[0] += any > 0.0 ? 1.0 : 0.0;
  }
  GLX_SGL_LOOP_END
  grid_reduce<2, 0x0u>(acc, red);
}

// One workgroup. keep: a flag per row of the current problem (k_sgl_screen's). Thread t owns a
// contiguous chunk of the groups, hence of the rows; the chunks' kept rows and surviving groups are
// counted, scanned in thread order, and every thread writes its rows and groups from its offsets.
// Integers only and no atomics: the same output every run.
//   rows_out: the kept rows of the current problem, ascending, then -1 up to ecnt[3];
//   ptr_out (K + 1), w_out, gcn_out, map_out (K): the reduced problem's groups, those that keep a row;
//   gcn is carried over: ||A_[g] restricted to the kept rows||_F <= ||A_[g]||_F, so the group test with
//   the stored value is the weaker one and stays safe. map_out names groups of the full problem (map ==
//   NULL: the current problem is the full one). ecnt = [K, rows, rows, rows rounded up to 64].
__global__ __launch_bounds__(256) void k_sgl_expand(const int* __restrict__ keep, const int* __restrict__ ptr,
                                                    const double* __restrict__ wts, const double* __restrict__ gcn,
                                                    const int* __restrict__ map, int64_t G,
                                                    int* __restrict__ rows_out, int* __restrict__ ptr_out,
                                                    double* __restrict__ w_out, double* __restrict__ gcn_out,
                                                    int* __restrict__ map_out, int* __restrict__ ecnt) {
  __shared__ long long roff[257], goff[257];
  const int64_t C = (G + 255) / 256;
  const int64_t k0 = (int64_t)threadIdx.x * C < G ? (int64_t)threadIdx.x * C : G;
  const int64_t k1 = k0 + C < G ? k0 + C : G;
  long long nr = 0, ng = 0;
  for (int64_t k = k0; k < k1; ++k) {
    int cnt = 0;
    for (int i = ptr[k]; i < ptr[k + 1]; ++i) cnt += keep[i];
    nr += cnt;
    ng += cnt > 0 ? 1 : 0;
  }
  roff[threadIdx.x] = nr;
  goff[threadIdx.x] = ng;
  __syncthreads();
  if (threadIdx.x == 0) {   // 256 chunk offsets, in thread order
    long long rr = 0, gg = 0;
    for (int t = 0; t < 256; ++t) {
      const long long a = roff[t], b = goff[t];
      roff[t] = rr;
      goff[t] = gg;
      rr += a;
      gg += b;
    }
    roff[256] = rr;
    goff[256] = gg;
  }
  __syncthreads();
  long long ro = roff[threadIdx.x], go = goff[threadIdx.x];
  for (int64_t k = k0; k < k1; ++k) {
    const long long start = ro;
    for (int i = ptr[k]; i < ptr[k + 1]; ++i)
      if (keep[i] != 0) rows_out[ro++] = i;
    if (ro > start) {
      ptr_out[go] = (int)start;
      w_out[go] = wts[k];
      gcn_out[go] = gcn[k];
      map_out[go] = map != nullptr ? map[k] : (int)k;
      ++go;
    }
  }
  const long long total = roff[256], K = goff[256];
  const long long wp = (total + 63) / 64 * 64;
  for (long long q = total + threadIdx.x; q < wp; q += 256) rows_out[q] = -1;
  if (threadIdx.x == 0) {
    ptr_out[K] = (int)total;
    ecnt[0] = (int)K;
    ecnt[1] = (int)total;
    ecnt[2] = (int)total;
    ecnt[3] = (int)wp;
  }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
// F receives (lpr_constant, re_constant) for l columns: the smallest sub-team that holds a row
template <typename F>
static void sgl_dispatch(int64_t l, F&& f) {
#define GLX_SGL_LE(LPR, RE) f(std::integral_constant<int, LPR>{}, std::integral_constant<int, RE>{})
  if (l <= 4) GLX_SGL_LE(4, 1);
  else if (l <= 16) GLX_SGL_LE(16, 1);
  else if (l <= 32) GLX_SGL_LE(32, 1);
  else if (l <= 64) GLX_SGL_LE(64, 1);
  else GLX_SGL_LE(64, 2);
#undef GLX_SGL_LE
}
std::string sgl_layout(int64_t l) {
  std::string s;
  sgl_dispatch(l, [&](auto lpr, auto re) {
    const int L = decltype(lpr)::value, E = decltype(re)::value;
    s = "a wave per group, " + std::to_string(L) + " lanes per row, " + std::to_string(E) +
        " element(s) per lane, two sweeps";
  });
  return s;
}

static void sgl_check(int64_t G, int64_t nrows, int64_t l) {
  if (G < 1 || nrows < 1) throw Error{GLX_E_INVALID, "sparse-group kernels: G and rows must be positive"};
  if (l < 1 || l > kMaxL) throw Error{GLX_E_INVALID, "the sparse-group kernels take 1 <= l <= 128"};
}

template <typename T>
void launch_sgl_fista(const T* y, const T* g, int S, const T* xk, T* xc, T* vnext, T* ynext, const int* ptr,
                      const double* wts, int64_t G, int64_t nrows, int64_t l, double t, double mu, double tau,
                      double thres, double theta, double theta_next, Red red, hipStream_t st) {
  sgl_check(G, nrows, l);
  sgl_dispatch(l, [&](auto lpr, auto re) {
    constexpr int L = decltype(lpr)::value, E = decltype(re)::value;
    hipLaunchKernelGGL((k_sgl_fista<T, L, E>), dim3(sgl_grid(G)), dim3(256), 0, st, y, g, S, xk, xc, vnext, ynext,
                       ptr, wts, G, nrows, l, t, t * (tau * mu), t * ((1.0 - tau) * mu), tau, 1.0 - tau, thres, theta,
                       1.0 - theta_next, theta_next, red);
  });
}

template <typename T>
void launch_sgl_cert(const T* x, const T* g, int S, T* gout, double* rn, const int* ptr, const double* wts, int64_t G,
                     int64_t nrows, int64_t l, double mu, double tau, Red red, hipStream_t st) {
  sgl_check(G, nrows, l);
  sgl_dispatch(l, [&](auto lpr, auto re) {
    constexpr int L = decltype(lpr)::value, E = decltype(re)::value;
    hipLaunchKernelGGL((k_sgl_cert<T, L, E>), dim3(sgl_grid(G)), dim3(256), 0, st, x, g, S, gout, rn, ptr, wts, G,
                       nrows, l, tau * mu, (1.0 - tau) * mu, tau, 1.0 - tau, red);
  });
}

void launch_sgl_dual_scale(const double* rho, const int* ptr, const double* wts, int64_t G, double a, double cb,
                           double mul0, double add0, double mul1, double add1, const double* rr, double* sg, Red red,
                           hipStream_t st) {
  if (G < 1) throw Error{GLX_E_INVALID, "sparse-group kernels: G must be positive"};
  hipLaunchKernelGGL(k_sgl_dual_scale, dim3(sgl_grid(G)), dim3(256), 0, st, rho, ptr, wts, G, a, cb, mul0, add0, mul1,
                     add1, rr, sg, red);
}

void launch_sgl_screen(const double* rho, const double* cn, const double* gcn, const int* ptr, const double* wts,
                       int64_t G, double s, double mul, double add, const double* rr, double rad, double a_lo,
                       double cb_lo, int group_test, int* keep, int* gkeep, Red red, hipStream_t st) {
  if (G < 1) throw Error{GLX_E_INVALID, "sparse-group kernels: G must be positive"};
  hipLaunchKernelGGL(k_sgl_screen, dim3(sgl_grid(G)), dim3(256), 0, st, rho, cn, gcn, ptr, wts, G, s, mul, add, rr,
                     rad, a_lo, cb_lo, group_test, keep, gkeep, red);
}

void launch_sgl_expand(const int* keep, const int* ptr, const double* wts, const double* gcn, const int* map,
                       int64_t G, int* rows_out, int* ptr_out, double* w_out, double* gcn_out, int* map_out, int* ecnt,
                       hipStream_t st) {
  if (G < 1) throw Error{GLX_E_INVALID, "sparse-group kernels: G must be positive"};
  hipLaunchKernelGGL(k_sgl_expand, dim3(1), dim3(256), 0, st, keep, ptr, wts, gcn, map, G, rows_out, ptr_out, w_out,
                     gcn_out, map_out, ecnt);
}

#define GLX_SGL_INST(T)                                                                                          \
  template void launch_sgl_fista<T>(const T*, const T*, int, const T*, T*, T*, T*, const int*, const double*,     \
                                    int64_t, int64_t, int64_t, double, double, double, double, double, double,    \
                                    Red, hipStream_t);                                                            \
  template void launch_sgl_cert<T>(const T*, const T*, int, T*, double*, const int*, const double*, int64_t,      \
                                   int64_t, int64_t, double, double, Red, hipStream_t);

GLX_SGL_INST(double)
GLX_SGL_INST(float)

}  // namespace glx
