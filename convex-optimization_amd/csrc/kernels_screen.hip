// kernels_screen.hip — the kernels of gap-safe screening (DESIGN.md "Certified solve and screening"):
//   k_col_norms    ||a_i||_2 of every column of row-major A in one coalesced pass, accumulated in
//                  double over fixed row slabs; the last workgroup of a column block sums the slabs in
//                  slab order and the grid reduction gives max_i ||a_i|| and sum_i ||a_i||^2
//   k_col_norms_w  the same walk with a weight per row of A: sqrt(sum_j w_j A_ji^2)
//   k_screen       the test  s ||g_i|| + ||a_i|| rho < mu  per row, the keep mask, and the ascending
//                  list of kept rows by an ordered scan: wave ballots, their popcounts, block offsets
//   k_gather_cols  dst[r, j] = src[r, idx[j]] (0 where idx[j] < 0), 16-byte stores
//   k_gather_rows / k_scatter_rows / k_compose_list  the same lists applied to x (n x l), to the
//                  column norms, and to the list that maps a reduced problem back to the full one
// Everything is deterministic: no atomics on floating-point values; the counters that find a last
// workgroup are integers and whatever that workgroup reads it sums in a fixed order.
#include <cstdlib>
#include <type_traits>

#include "glx.h"
#include "glx_device.h"

namespace glx {

// ------------------------------------------------------------------------------------------
// column norms
// ------------------------------------------------------------------------------------------
// Row slabs of k_col_norms: at most 64, each at least 64 rows (a function of m alone, so the
// summation order is fixed by the shape).
int col_norm_slabs(int64_t m) {
  const int64_t sl = clampi(cdiv(m, 64), 1, 64);
  const int64_t rps = cdiv(m, sl);
  return (int)cdiv(m, rps);
}
static int64_t col_norm_rows_per_slab(int64_t m) { return cdiv(m, clampi(cdiv(m, 64), 1, 64)); }
static unsigned col_norm_blocks(int64_t n) { return (unsigned)clampi(cdiv(n, 256), 1, kMaxBlocks); }
size_t col_norms_part_bytes(int64_t m, int64_t n) { return sizeof(double) * (size_t)col_norm_slabs(m) * (size_t)n; }
size_t col_norms_count_bytes(int64_t n) { return sizeof(unsigned) * (size_t)col_norm_blocks(n); }

// grid (column blocks, slabs). Lane j of a column block owns columns j, j + 256 gridDim.x, ...:
// adjacent lanes read adjacent columns of one row, four rows in flight.
template <typename T>
__global__ __launch_bounds__(256) void k_col_norms(const T* __restrict__ A, int64_t m, int64_t n, int64_t rps,
                                                   double* __restrict__ part, unsigned* __restrict__ ccnt,
                                                   double* __restrict__ norms, Red red) {
  __shared__ int last;
  const int64_t r0 = (int64_t)blockIdx.y * rps;
  const int64_t r1 = r0 + rps < m ? r0 + rps : m;
  const int64_t cstride = (int64_t)gridDim.x * 256;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += cstride) {
    const T* p = A + r0 * n + j;
    double acc = 0.0;
    int64_t r = r0;
    for (; r + 4 <= r1; r += 4) {
      const double a0 = (double)p[0], a1 = (double)p[n], a2 = (double)p[2 * n], a3 = (double)p[3 * n];
      acc += a0 * a0;
      acc += a1 * a1;
      acc += a2 * a2;
      acc += a3 * a3;
      p += 4 * n;
    }
    for (; r < r1; ++r) {
      const double a0 = (double)p[0];
      acc += a0 * a0;
      p += n;
    }
    __hip_atomic_store(part + (int64_t)blockIdx.y * n + j, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // write-through stores drained before the arrival (kernels_atr.hip atr_split_combine)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned arrival = __hip_atomic_fetch_add(ccnt + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = arrival == gridDim.y - 1;
  }
  __syncthreads();
  if (!last) return;
  double v[2] = {-__builtin_inf(), 0.0};
  const int S = (int)gridDim.y;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += cstride) {
    double s = 0.0;
    for (int k = 0; k < S; ++k)
      s += __hip_atomic_load(part + (int64_t)k * n + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double nrm = __builtin_sqrt(s);
    norms[j] = nrm;
    v[0] = nan_max(v[0], nrm);
    v[1] += s;
  }
  if (threadIdx.x == 0) __hip_atomic_store(ccnt + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  grid_reduce<2, 0x1u>(v, red, (int)blockIdx.x, (int)gridDim.x);
}

// The weighted norms sqrt(sum_j w_j A_ji^2) of the sample-weighted problem (DESIGN.md "Sample weights
// and cross-validation"): k_col_norms' walk, slabs and last-block combine, kept as a sibling so that
// k_col_norms stays instruction for instruction (a shared inlined body did not compile to the same
// code). w_j is uniform over a wave (a lane owns a column): one broadcast load per row. The term is
// (w a) a, which is a a exactly for w = 1 and 0 for w = 0.
template <typename T>
__global__ __launch_bounds__(256) void k_col_norms_w(const T* __restrict__ A, const T* __restrict__ w, int64_t m,
                                                     int64_t n, int64_t rps, double* __restrict__ part,
                                                     unsigned* __restrict__ ccnt, double* __restrict__ norms,
                                                     Red red) {
  __shared__ int last;
  const int64_t r0 = (int64_t)blockIdx.y * rps;
  const int64_t r1 = r0 + rps < m ? r0 + rps : m;
  const int64_t cstride = (int64_t)gridDim.x * 256;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += cstride) {
    const T* p = A + r0 * n + j;
    double acc = 0.0;
    int64_t r = r0;
    for (; r + 4 <= r1; r += 4) {
      const double a0 = (double)p[0], a1 = (double)p[n], a2 = (double)p[2 * n], a3 = (double)p[3 * n];
      acc += ((double)w[r] * a0) * a0;
      acc += ((double)w[r + 1] * a1) * a1;
      acc += ((double)w[r + 2] * a2) * a2;
      acc += ((double)w[r + 3] * a3) * a3;
      p += 4 * n;
    }
    for (; r < r1; ++r) {
      const double a0 = (double)p[0];
      acc += ((double)w[r] * a0) * a0;
      p += n;
    }
    __hip_atomic_store(part + (int64_t)blockIdx.y * n + j, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned arrival = __hip_atomic_fetch_add(ccnt + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = arrival == gridDim.y - 1;
  }
  __syncthreads();
  if (!last) return;
  double v[2] = {-__builtin_inf(), 0.0};
  const int S = (int)gridDim.y;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += cstride) {
    double s = 0.0;
    for (int k = 0; k < S; ++k)
      s += __hip_atomic_load(part + (int64_t)k * n + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double nrm = __builtin_sqrt(s);
    norms[j] = nrm;
    v[0] = nan_max(v[0], nrm);
    v[1] += s;
  }
  if (threadIdx.x == 0) __hip_atomic_store(ccnt + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  grid_reduce<2, 0x1u>(v, red, (int)blockIdx.x, (int)gridDim.x);
}

// The centred weighted column norms of the problem with an intercept (DESIGN.md "Intercept"), two
// launches on k_col_norms' walk, slabs and last-block combine, siblings again (w == NULL: unit weights):
//   k_col_means    mean[i] = sum_j w_j A_ji / sigma; the grid reduction gives max_i |mean[i]| and
//                  sum_i mean[i]^2 (the guard recovers the uncentred norms from them)
//   k_col_norms_c  sqrt(sum_j w_j (A_ji - mean[i])^2), the difference taken in double, the term formed
//                  as (w d) d; max and sum of squares as k_col_norms
// Any mean other than the exact one only enlarges the second sum, so its rounding errs on the safe side.
template <typename T>
__global__ __launch_bounds__(256) void k_col_means(const T* __restrict__ A, const T* __restrict__ w, int64_t m,
                                                   int64_t n, int64_t rps, double sigma, double* __restrict__ part,
                                                   unsigned* __restrict__ ccnt, double* __restrict__ mean, Red red) {
  __shared__ int last;
  const int64_t r0 = (int64_t)blockIdx.y * rps;
  const int64_t r1 = r0 + rps < m ? r0 + rps : m;
  const int64_t cstride = (int64_t)gridDim.x * 256;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += cstride) {
    const T* p = A + r0 * n + j;
    double acc = 0.0;
    int64_t r = r0;
    for (; r + 4 <= r1; r += 4) {
      const double a0 = (double)p[0], a1 = (double)p[n], a2 = (double)p[2 * n], a3 = (double)p[3 * n];
      acc += (w != nullptr ? (double)w[r] : 1.0) * a0;
      acc += (w != nullptr ? (double)w[r + 1] : 1.0) * a1;
      acc += (w != nullptr ? (double)w[r + 2] : 1.0) * a2;
      acc += (w != nullptr ? (double)w[r + 3] : 1.0) * a3;
      p += 4 * n;
    }
    for (; r < r1; ++r) {
      acc += (w != nullptr ? (double)w[r] : 1.0) * (double)p[0];
      p += n;
    }
    __hip_atomic_store(part + (int64_t)blockIdx.y * n + j, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned arrival = __hip_atomic_fetch_add(ccnt + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = arrival == gridDim.y - 1;
  }
  __syncthreads();
  if (!last) return;
  double v[2] = {-__builtin_inf(), 0.0};
  const int S = (int)gridDim.y;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += cstride) {
    double s = 0.0;
    for (int k = 0; k < S; ++k)
      s += __hip_atomic_load(part + (int64_t)k * n + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double mu = s / sigma;
    mean[j] = mu;
    v[0] = nan_max(v[0], mu < 0.0 ? -mu : mu);
    v[1] += mu * mu;
  }
  if (threadIdx.x == 0) __hip_atomic_store(ccnt + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  grid_reduce<2, 0x1u>(v, red, (int)blockIdx.x, (int)gridDim.x);
}

template <typename T>
__global__ __launch_bounds__(256) void k_col_norms_c(const T* __restrict__ A, const T* __restrict__ w,
                                                     const double* __restrict__ mean, int64_t m, int64_t n,
                                                     int64_t rps, double* __restrict__ part,
                                                     unsigned* __restrict__ ccnt, double* __restrict__ norms,
                                                     Red red) {
  __shared__ int last;
  const int64_t r0 = (int64_t)blockIdx.y * rps;
  const int64_t r1 = r0 + rps < m ? r0 + rps : m;
  const int64_t cstride = (int64_t)gridDim.x * 256;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += cstride) {
    const T* p = A + r0 * n + j;
    const double mj = mean[j];
    double acc = 0.0;
    int64_t r = r0;
    for (; r + 4 <= r1; r += 4) {
      const double d0 = (double)p[0] - mj, d1 = (double)p[n] - mj, d2 = (double)p[2 * n] - mj,
                   d3 = (double)p[3 * n] - mj;
      acc += ((w != nullptr ? (double)w[r] : 1.0) * d0) * d0;
      acc += ((w != nullptr ? (double)w[r + 1] : 1.0) * d1) * d1;
      acc += ((w != nullptr ? (double)w[r + 2] : 1.0) * d2) * d2;
      acc += ((w != nullptr ? (double)w[r + 3] : 1.0) * d3) * d3;
      p += 4 * n;
    }
    for (; r < r1; ++r) {
      const double d0 = (double)p[0] - mj;
      acc += ((w != nullptr ? (double)w[r] : 1.0) * d0) * d0;
      p += n;
    }
    __hip_atomic_store(part + (int64_t)blockIdx.y * n + j, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned arrival = __hip_atomic_fetch_add(ccnt + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = arrival == gridDim.y - 1;
  }
  __syncthreads();
  if (!last) return;
  double v[2] = {-__builtin_inf(), 0.0};
  const int S = (int)gridDim.y;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += cstride) {
    double s = 0.0;
    for (int k = 0; k < S; ++k)
      s += __hip_atomic_load(part + (int64_t)k * n + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double nrm = __builtin_sqrt(s);
    norms[j] = nrm;
    v[0] = nan_max(v[0], nrm);
    v[1] += s;
  }
  if (threadIdx.x == 0) __hip_atomic_store(ccnt + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  grid_reduce<2, 0x1u>(v, red, (int)blockIdx.x, (int)gridDim.x);
}

// mean: n doubles; red_mean.out = [max_i |mean[i]|, sum_i mean[i]^2]; red.out as launch_col_norms'
template <typename T>
void launch_col_norms_c(const T* A, const T* w, double sigma, int64_t m, int64_t n, double* norms, double* mean,
                        double* part, unsigned* ccnt, Red red_mean, Red red, hipStream_t st) {
  const dim3 grid(col_norm_blocks(n), (unsigned)col_norm_slabs(m));
  hipLaunchKernelGGL(k_col_means<T>, grid, dim3(256), 0, st, A, w, m, n, col_norm_rows_per_slab(m), sigma, part, ccnt,
                     mean, red_mean);
  hipLaunchKernelGGL(k_col_norms_c<T>, grid, dim3(256), 0, st, A, w, mean, m, n, col_norm_rows_per_slab(m), part, ccnt,
                     norms, red);
}

template <typename T>
void launch_col_norms(const T* A, int64_t m, int64_t n, double* norms, double* part, unsigned* ccnt, Red red,
                      hipStream_t st) {
  const dim3 grid(col_norm_blocks(n), (unsigned)col_norm_slabs(m));
  hipLaunchKernelGGL(k_col_norms<T>, grid, dim3(256), 0, st, A, m, n, col_norm_rows_per_slab(m), part, ccnt,
                     norms, red);
}
template <typename T>
void launch_col_norms_w(const T* A, const T* w, int64_t m, int64_t n, double* norms, double* part, unsigned* ccnt,
                        Red red, hipStream_t st) {
  const dim3 grid(col_norm_blocks(n), (unsigned)col_norm_slabs(m));
  hipLaunchKernelGGL(k_col_norms_w<T>, grid, dim3(256), 0, st, A, w, m, n, col_norm_rows_per_slab(m), part, ccnt,
                     norms, red);
}

// ------------------------------------------------------------------------------------------
// the screening test and the ordered list of kept rows
// ------------------------------------------------------------------------------------------
static unsigned screen_blocks(int64_t n) { return (unsigned)clampi(cdiv(n, 256), 1, kMaxBlocks); }
size_t screen_words_bytes(int64_t n) { return sizeof(unsigned long long) * (size_t)(cdiv(n, 64) + 1); }

// Row i is screened (keep = 0) exactly when  s rn[i] + cn[i] rho < mu_lo  holds; a NaN in any of
// them fails the comparison and keeps the row. Whole waves walk the rows up to n rounded up to 64,
// so every ballot is of a full wave and word w of `bal` holds rows 64 w .. 64 w + 63. The last
// workgroup to arrive turns the words into the list: thread t owns a contiguous run of words, the
// runs' popcounts are scanned in thread order, and every thread emits its rows in ascending order
// from its offset. cnt = [kept, kept rounded up to 64]; list[kept .. cnt[1]) = -1.
__global__ __launch_bounds__(256) void k_screen(const double* __restrict__ rn, const double* __restrict__ cn,
                                                int64_t n, double s, double rho, double mu_lo,
                                                unsigned char* __restrict__ mask, int* __restrict__ list,
                                                int* __restrict__ cnt, unsigned long long* __restrict__ bal,
                                                unsigned* __restrict__ ticket) {
  __shared__ int last;
  __shared__ long long offs[257];
  const int lane = threadIdx.x & 63;
  const int64_t npad = (n + 63) / 64 * 64;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npad; i += stride) {
    bool keep = false;
    if (i < n) {
      const double lhs = s * rn[i] + cn[i] * rho;
      keep = !(lhs < mu_lo);
      if (mask != nullptr) mask[i] = keep ? 1 : 0;
    }
    const unsigned long long b = __ballot(keep);
    if (lane == 0) __hip_atomic_store(bal + i / 64, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned arrival = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = arrival == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  const int64_t W = npad / 64;
  const int64_t C = (W + 255) / 256;
  const int64_t w0 = (int64_t)threadIdx.x * C < W ? (int64_t)threadIdx.x * C : W;
  const int64_t w1 = w0 + C < W ? w0 + C : W;
  long long c = 0;
  for (int64_t w = w0; w < w1; ++w)
    c += __popcll(__hip_atomic_load(bal + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  offs[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {   // 256 block offsets, in thread order
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
  for (int64_t w = w0; w < w1; ++w) {
    unsigned long long b = __hip_atomic_load(bal + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (b != 0ull) {
      const int j = __ffsll((long long)b) - 1;
      list[o++] = (int)(w * 64 + j);
      b &= b - 1ull;
    }
  }
  const long long total = offs[256];
  const long long wp = (total + 63) / 64 * 64;
  for (long long q = total + threadIdx.x; q < wp; q += 256) list[q] = -1;
  if (threadIdx.x == 0) {
    cnt[0] = (int)total;
    cnt[1] = (int)wp;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

void launch_screen(const double* rn, const double* cn, int64_t n, double s, double rho, double mu_lo,
                   unsigned char* mask, int* list, int* cnt, unsigned long long* bal, unsigned* ticket,
                   hipStream_t st) {
  hipLaunchKernelGGL(k_screen, dim3(screen_blocks(n)), dim3(256), 0, st, rn, cn, n, s, rho, mu_lo, mask, list,
                     cnt, bal, ticket);
}

// ------------------------------------------------------------------------------------------
// gathers
// ------------------------------------------------------------------------------------------
template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) GVec {
  T v[VEC];
};

// grid (column groups, row walkers): a thread owns VEC adjacent destination columns (adjacent lanes
// adjacent groups, so the ascending list keeps a wave's reads inside as few lines of src as its
// gaps allow) and walks the rows gridDim.y apart. wp is a multiple of 64, so with VEC > 1 every
// row of dst starts 16-byte aligned where dst does. An index outside [0, sw) gives 0.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_gather_cols(const T* __restrict__ src, int64_t m, int64_t sw,
                                                     const int* __restrict__ idx, int64_t wp,
                                                     T* __restrict__ dst) {
  const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (j0 >= wp) return;
  int64_t id[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const int k = idx[j0 + e];
    id[e] = (k >= 0 && (int64_t)k < sw) ? (int64_t)k : (int64_t)-1;
  }
#pragma unroll 4
  for (int64_t r = blockIdx.y; r < m; r += gridDim.y) {
    const T* row = src + r * sw;
    GVec<T, VEC> o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) o.v[e] = id[e] >= 0 ? row[id[e]] : T(0);
    *reinterpret_cast<GVec<T, VEC>*>(dst + r * wp + j0) = o;
  }
}

template <typename T>
void launch_gather_cols(const T* src, int64_t m, int64_t sw, const int* idx, int64_t wp, T* dst, hipStream_t st) {
  if (wp <= 0 || m <= 0) return;
  if (wp % 64 != 0) throw Error{GLX_E_INVALID, "gather: the padded width must be a multiple of 64"};
  constexpr int V = 16 / (int)sizeof(T);
  const bool vec = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const int v = vec ? V : 1;
  const unsigned gx = (unsigned)cdiv(wp, 256 * (int64_t)v);
  const unsigned gy = (unsigned)clampi(cdiv(4096, gx), 1, m < 1024 ? m : 1024);
  if (vec) hipLaunchKernelGGL((k_gather_cols<T, V>), dim3(gx, gy), dim3(256), 0, st, src, m, sw, idx, wp, dst);
  else hipLaunchKernelGGL((k_gather_cols<T, 1>), dim3(gx, gy), dim3(256), 0, st, src, m, sw, idx, wp, dst);
}

// dst[j, :] = src[idx[j], :] (0 where idx[j] < 0), j < wp, rows of l values
template <typename T>
__global__ __launch_bounds__(256) void k_gather_rows(const T* __restrict__ src, const int* __restrict__ idx,
                                                     int64_t wp, int64_t l, T* __restrict__ dst) {
  const int64_t tot = wp * l;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
    const int64_t j = e / l, c = e - j * l;
    const int k = idx[j];
    dst[e] = k >= 0 ? src[(int64_t)k * l + c] : T(0);
  }
}
// dst[idx[j], :] = src[j, :] where idx[j] >= 0 (the caller clears dst first)
template <typename T>
__global__ __launch_bounds__(256) void k_scatter_rows(const T* __restrict__ src, const int* __restrict__ idx,
                                                      int64_t wp, int64_t l, T* __restrict__ dst) {
  const int64_t tot = wp * l;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
    const int64_t j = e / l, c = e - j * l;
    const int k = idx[j];
    if (k >= 0) dst[(int64_t)k * l + c] = src[e];
  }
}
// out[j] = map[idx[j]] (idx[j] where map == NULL: the first list), -1 where idx[j] < 0
__global__ __launch_bounds__(256) void k_compose_list(const int* __restrict__ map, const int* __restrict__ idx,
                                                      int64_t wp, int* __restrict__ out) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < wp; j += (int64_t)gridDim.x * 256) {
    const int k = idx[j];
    out[j] = k < 0 ? -1 : (map != nullptr ? map[k] : k);
  }
}

static unsigned rows_grid(int64_t work) { return (unsigned)clampi(cdiv(work, 256), 1, 4096); }
template <typename T>
void launch_gather_rows(const T* src, const int* idx, int64_t wp, int64_t l, T* dst, hipStream_t st) {
  if (wp <= 0) return;
  hipLaunchKernelGGL(k_gather_rows<T>, dim3(rows_grid(wp * l)), dim3(256), 0, st, src, idx, wp, l, dst);
}
template <typename T>
void launch_scatter_rows(const T* src, const int* idx, int64_t wp, int64_t l, T* dst, hipStream_t st) {
  if (wp <= 0) return;
  hipLaunchKernelGGL(k_scatter_rows<T>, dim3(rows_grid(wp * l)), dim3(256), 0, st, src, idx, wp, l, dst);
}
void launch_compose_list(const int* map, const int* idx, int64_t wp, int* out, hipStream_t st) {
  if (wp <= 0) return;
  hipLaunchKernelGGL(k_compose_list, dim3(rows_grid(wp)), dim3(256), 0, st, map, idx, wp, out);
}

#define GLX_SCREEN_INST(T)                                                                                  \
  template void launch_col_norms<T>(const T*, int64_t, int64_t, double*, double*, unsigned*, Red, hipStream_t); \
  template void launch_col_norms_w<T>(const T*, const T*, int64_t, int64_t, double*, double*, unsigned*, Red, \
                                      hipStream_t);                                                         \
  template void launch_col_norms_c<T>(const T*, const T*, double, int64_t, int64_t, double*, double*, double*, \
                                      unsigned*, Red, Red, hipStream_t);                                    \
  template void launch_gather_cols<T>(const T*, int64_t, int64_t, const int*, int64_t, T*, hipStream_t);     \
  template void launch_gather_rows<T>(const T*, const int*, int64_t, int64_t, T*, hipStream_t);             \
  template void launch_scatter_rows<T>(const T*, const int*, int64_t, int64_t, T*, hipStream_t);

GLX_SCREEN_INST(double)
GLX_SCREEN_INST(float)

}  // namespace glx
