// kernels_atr.hip — the gradient contraction A^T R (reference: gl_ProxGD_primal.py:129
// `A.T @ (A @ x - b)`; gl_FProxGD_primal.py:65-66) on MFMA, with the ProxGD / FISTA line-search
// trial fused into its epilogue (k_atr_prox, k_atr_fista), and the VALU fallback for small l.
//
// The K index (rows of A) is on l>>4 and the 16-wide M index (columns of A) on l&15, so lanes
// 0..15 read consecutive columns: a lane loads 4 columns of one row (atr_col) and feeds 4 MFMAs
// whose output rows are those columns. Split-K partials (waves through LDS, workgroups as
// slabs) are summed in a fixed order, so every result is deterministic run to run.
#include <cstdio>

#include "glx_mfma.h"

namespace glx {

// ------------------------------------------------------------------------------------------
// A^T R on MFMA: a wave owns 64 columns of A (= 64 rows of G) x NT 16-col tiles of G.
//   WL = 0: a block = one 64-column panel, its 4 waves split the block's rows (LDS-reduced);
//   WL = 1: a block = four adjacent panels (256 columns) sharing one row range, so the four
//           waves read the same R fragments (L1 hits) and write their slabs directly;
//   WL = 2: as WL 0 with eight waves (512 threads, two waves per SIMD): the block's rows split
//           eight ways, waves 4..7 folded into 0..3 through LDS first (round 4);
//   WL = 3: as WL 0 with a 32-column panel (f64; round 5): twice the panels, so a shape with
//           n / 64 < 256 (C2: 128) fills the chip without K splits and their slab combine.
// blockIdx.y = row split. Needs n % 64 == 0 (n % 256 for WL = 1), m % 4 == 0.
// Gp[split][n][16*NT].
// ------------------------------------------------------------------------------------------
// One 64-column panel of A^T R over this wave's (WL 1: this block's) row range; returns the
// panel's first column. acc[e][nt] holds rows col0 + atr_col(M::row(lane, r), e). For WL 0 the
// block's four waves split the rows (K) and are summed through LDS in the fixed order
// ((w0 + w1) + w2) + w3; afterwards wave w holds the complete sum for e == w in acc[w][*]
// (the other e of a wave are partial and unused), so the four waves share the epilogue.
// (pbx, pby) = (panel, K split) of this block: (blockIdx.x, blockIdx.y) for k_atr_mfma.
// Infinity-Cache hand-off (GemmPlan::atr_keep_mib, a kernel argument; the solver's default is
// kKeepMiB = 192, GLX_ATR_KEEP_MIB overrides it, 0 = off): the last rows a non-temporal A^T R
// pass reads are loaded with the default policy, so that about that many MiB of A stay in the
// 256 MiB Infinity Cache for the next pass over A (A@X) to hit.

// panel width (columns of A = rows of G) of a wave layout, and its MFMA output groups e
template <int WL> constexpr int atr_pw() { return (WL == 3 || WL == 4) ? 32 : 64; }
// waves per workgroup: WL 2 (64-column panel) and WL 4 (32-column panel, round 5) have eight
template <int WL> constexpr int atr_waves() { return (WL == 2 || WL == 4) ? 8 : 4; }
template <int WL> constexpr int atr_ne() { return atr_pw<WL>() / 16; }

// head (round 8, k_atr_prox's finalize head): a callable every thread of the workgroup runs once
// the ring's first PF A loads are in flight and before any load of R (it produces R and holds
// workgroup barriers); false from it: the panel is abandoned and -1 returned.
// (R is written by the head, so only the plain form declares it __restrict__.)
template <typename T, bool HEAD> struct AtrRPtr { typedef const T* __restrict__ type; };
template <typename T> struct AtrRPtr<T, true> { typedef const T* type; };
template <typename T, int NT, int PF, int WL, bool NTL, typename HeadFn = std::nullptr_t>
__device__ inline int64_t atr_panel(const T* __restrict__ A,
                                    typename AtrRPtr<T, !std::is_same<HeadFn, std::nullptr_t>::value>::type R, int64_t m,
                                    int64_t n, int S, typename MF<T>::acc_t (&acc)[4][NT],
                                    int64_t pbx, int64_t pby, int keep_mib, HeadFn head = nullptr) {
  constexpr bool HEAD = !std::is_same<HeadFn, std::nullptr_t>::value;
  typedef MF<T> M;
  typedef typename M::acc_t C;
  constexpr int L = 16 * NT;
  constexpr bool RW = WL != 1;   // the block's waves split the rows of one panel
  constexpr int NWV = atr_waves<WL>();
  constexpr int PW = atr_pw<WL>(), NE = atr_ne<WL>();
  static_assert((WL != 3 && WL != 4) || sizeof(T) == 8, "the 32-column panel is f64 (one 16-B load per row)");
  __shared__ C red[RW ? 4 : 1][RW ? 4 * NT : 1][64];   // [wave][e * NT + nt][lane]

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int64_t col0 = RW ? pbx * PW : pbx * 256 + wave * 64;
  const int64_t steps = m / 4;
  const int64_t W = RW ? (int64_t)S * NWV : (int64_t)S;
  const int64_t w = RW ? pby * NWV + wave : pby;
  const int64_t sb = steps * w / W, se = steps * (w + 1) / W;

  const T* ap = A + (sb * 4 + q) * n + col0 + atr_col<T>(i, 0);
  const T* rp = R + (sb * 4 + q) * L + i;

#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[e][nt] = C{};

  // Ring of PF row steps, consumed in place: a step's fragments feed its MFMAs and are then
  // refilled with step s + PF in the same registers, at a clamped offset so that the main
  // loop carries no load predicates (a predicate or a register copy at the loop's back edge
  // makes the compiler drain vmcnt to 0 there). Lookahead = PF - 1 steps.
  const int64_t nst = se - sb;
  T a[PF][4], rb[PF][NT];
  auto lda = [&](const T* p, T (&dst)[4], auto ntl) {
    if constexpr (NE == 2) {   // columns 2i, 2i + 1 (atr_col for e < 2): one 16-B load
      const typename M::vec_t v = load_vec<T, decltype(ntl)::value>(p);
      dst[0] = v[0];
      dst[1] = v[1];
    } else {
      Load4<T, decltype(ntl)::value>::go(p, dst);
    }
  };
  auto ld = [&](int p, int64_t off) {
    off = off < nst ? off : nst - 1;
    lda(ap + off * 4 * n, a[p], std::integral_constant<bool, NTL>{});
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) rb[p][nt] = rp[off * 4 * L + nt * 16];
  };
  auto ld_def = [&](int p, int64_t off) {   // default policy (the Infinity-Cache hand-off)
    off = off < nst ? off : nst - 1;
    lda(ap + off * 4 * n, a[p], std::integral_constant<bool, false>{});
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) rb[p][nt] = rp[off * 4 * L + nt * 16];
  };
  // steps [kt, nst) load with the default policy: keep MiB over the grid's W * (n / 64) waves of
  // 4 rows x 64 columns per step (WL 1: 4 x 256 columns per block step)
  int64_t keep = 0;
  if constexpr (NTL) {
    const int64_t kb = (int64_t)keep_mib << 20;
    keep = kb / ((int64_t)(RW ? W * (n / PW) : W * (n / 256)) * 4 * (RW ? PW : 256) * (int64_t)sizeof(T));
  }
  const int64_t kt = nst - keep;
  auto mma_step = [&](int p) {
#pragma unroll
    for (int e = 0; e < NE; ++e)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[e][nt] = M::mma(a[p][e], rb[p][nt], acc[e][nt]);
  };
  GLX_CLK(1);
  if constexpr (HEAD) {
    if (nst > 0) {
#pragma unroll
      for (int p = 0; p < PF; ++p)
        lda(ap + (p < nst ? p : nst - 1) * 4 * n, a[p], std::integral_constant<bool, NTL>{});
    }
    if (!head()) return -1;
    if (nst > 0) {
#pragma unroll
      for (int p = 0; p < PF; ++p)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) rb[p][nt] = rp[(p < nst ? p : nst - 1) * 4 * L + nt * 16];
    }
  }
  if (nst > 0) {
    if constexpr (!HEAD) {
#pragma unroll
      for (int p = 0; p < PF; ++p) ld(p, p);
    }
    // Trip bounds as wave-uniform 32-bit scalars (readfirstlane): round 3's fused condition
    // `s0 + PF <= nst && (keep == 0 || s0 + 2 PF <= kt)` compiled into an exec-masked loop with
    // an s_nop per MFMA group, and k_atr_prox ran 180 us against round 2's 168 us on one box
    // (profiles/r4_diag/). Loop 1 runs while s0 + PF <= min(nst, kt - PF).
    const int nsti = __builtin_amdgcn_readfirstlane((int)nst);
    const int lim1 = __builtin_amdgcn_readfirstlane(
        keep == 0 ? (int)nst : (int)(kt - PF < nst ? kt - PF : nst));
    int s0 = 0;
    for (; s0 + PF <= lim1; s0 += PF) {
#pragma unroll
      for (int p = 0; p < PF; ++p) {
        mma_step(p);
        ld(p, s0 + p + PF);
      }
    }
    for (; s0 + PF <= nsti; s0 += PF) {   // the kept tail (only with keep > 0)
#pragma unroll
      for (int p = 0; p < PF; ++p) {
        mma_step(p);
        ld_def(p, s0 + p + PF);
      }
    }
#pragma unroll
    for (int p = 0; p < PF - 1; ++p)
      if (s0 + p < nst) mma_step(p);
  }
  GLX_CLK(2);

  if constexpr (WL == 2 || WL == 4) {   // waves 4..7 into 0..3: acc(w) + acc(w + 4)
    if (wave >= 4) {
#pragma unroll
      for (int e = 0; e < NE; ++e)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) red[wave - 4][e * NT + nt][lane] = acc[e][nt];
    }
    __syncthreads();
    if (wave < 4) {
#pragma unroll
      for (int e = 0; e < NE; ++e)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[e][nt] += red[wave][e * NT + nt][lane];
    }
    __syncthreads();
  }
  if (RW) {
    if (wave < 4) {
#pragma unroll
      for (int e = 0; e < NE; ++e)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) red[wave][e * NT + nt][lane] = acc[e][nt];
    }
    __syncthreads();
    if (wave < NE) {   // (WL 2: waves 4..7 hold no rows from here on; WL 3: waves 2, 3)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        C v = red[0][wave * NT + nt][lane];
#pragma unroll
        for (int s = 1; s < 4; ++s) v += red[s][wave * NT + nt][lane];
#pragma unroll
        for (int e = 0; e < NE; ++e)
          if (e == wave) acc[e][nt] = v;   // static register index; e == wave selects one
      }
    }
  }
  return col0;
}

// K splits of a fused A^T R (WL 0, S > 1): a 1-D grid of n/64 panels x S splits (+ the
// publisher). Every block stores its panel rows (wave w: rows e == w) into slab `split` of Gp;
// the block that arrives last on its panel's counter sums the S slabs in slab order (the
// order of slab_sum, so G is bit-identical to the unfused path) and runs the trial epilogue.
// Hand-off: sc1 (agent-scope) stores, vmcnt(0), a workgroup barrier, one agent-scope add per
// block; the last arriver loads with sc1 after a barrier (MI355X_MICROARCH.md "Valid forms",
// row 1). Returns false in the blocks that are not last: they leave the kernel without joining
// the grid reduction, which counts only the n/64 panel owners (+ the publisher; grid_reduce's
// nparts), so S is not bounded by the kMaxBlocks partials row (round 3: C2 takes more splits).
// *slot = the panel: the trial's scalar sums come out in panel order, bit-identical from run to
// run whatever the arrival order (a last arriver at its own block slot made their summation
// order depend on timing), and equal to the earlier form that also reduced identity partials.
template <typename T, int NT>
__device__ inline bool atr_split_combine(typename MF<T>::acc_t (&acc)[4][NT], T* __restrict__ Gp,
                                         int64_t n, int S, int64_t panel, int64_t split,
                                         unsigned* __restrict__ pcnt, int* slot) {
  typedef MF<T> M;
  constexpr int L = 16 * NT;
  __shared__ int last;
  __shared__ unsigned arrival;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i = lane & 15;
  const int64_t col0 = panel * 64;
  const int64_t nl = n * L;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e != wave) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = col0 + atr_col<T>(M::row(lane, r), e);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        __hip_atomic_store(Gp + split * nl + row * L + nt * 16 + i, acc[e][nt][r], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    arrival = __hip_atomic_fetch_add(pcnt + panel, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = arrival == (unsigned)S - 1;
  }
  __syncthreads();
  if (!last) return false;
  *slot = (int)panel;
  // Round 5: every slab load of the wave's 4 x NT elements issued before the first add (S <= 8,
  // atr_prox_ok), one round trip instead of S - 1 dependent ones per element; same slab order
  constexpr int KS = NT == 1 ? 8 : 4;   // slabs per load batch (register budget)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e != wave) continue;
    for (int k0 = 0; k0 < S; k0 += KS) {
      T sv[4][NT][KS];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = col0 + atr_col<T>(M::row(lane, r), e);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const T* g = Gp + row * L + nt * 16 + i;
#pragma unroll
          for (int k = 0; k < KS; ++k)
            sv[r][nt][k] = k0 + k < S ? __hip_atomic_load(g + (int64_t)(k0 + k) * nl, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT)
                                      : T(0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          T v = k0 == 0 ? sv[r][nt][0] : acc[e][nt][r] + sv[r][nt][0];
#pragma unroll
          for (int k = 1; k < KS; ++k)
            if (k0 + k < S) v = v + sv[r][nt][k];
          acc[e][nt][r] = v;
        }
    }
  }
  if (threadIdx.x == 0) __hip_atomic_store(pcnt + panel, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

template <typename T, int NT, int PF, int WL, bool NTL>
__global__ __launch_bounds__(atr_waves<WL>() * 64) void k_atr_mfma(const T* __restrict__ A, const T* __restrict__ R,
                                                  T* __restrict__ Gp, int64_t m, int64_t n, int S,
                                                  int keep_mib) {
  typedef MF<T> M;
  constexpr int L = 16 * NT;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i = lane & 15;
  typename M::acc_t acc[4][NT];
  const int64_t col0 = atr_panel<T, NT, PF, WL, NTL>(A, R, m, n, S, acc, blockIdx.x, blockIdx.y, keep_mib);
  T* gout = Gp + (int64_t)blockIdx.y * n * L;
#pragma unroll
  for (int e = 0; e < atr_ne<WL>(); ++e) {
    if (WL != 1 && e != wave) continue;   // WL 0 / 2 / 3: wave w < NE owns the rows e == w
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t grow = col0 + atr_col<T>(M::row(lane, r), e);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) gout[grow * L + nt * 16 + i] = acc[e][nt][r];
    }
  }
}

// ------------------------------------------------------------------------------------------
// Round 8: the residual finalize at the head of k_atr_prox (FinHead, glx_internal.h): the launch's
// panel workgroups walk the finalize's 256-thread blocks (block w, w + nw, ...: fin_block_elems
// and grid_reduce's parts_only form, so every residual and every partial is the separate kernel's
// bit for bit) while their ring's first A loads are in flight. Opt-in (GLX_FIN_HEAD=1): at NS the
// four blocks a workgroup walks in series, 19 loads per thread each, and the hand-off cost 20 us
// where k_finalize_residual costs 13 ("Round 8").
// Hand-off (MI355X_MICROARCH.md, visibility "Valid forms"): write-through (sc1) stores of R and
// the partials, vmcnt(0), a workgroup barrier, one agent-scope add per workgroup on the sharded
// ticket; then one lane polls the final counter with sc1 loads (s_sleep between polls, bounded by
// s_memrealtime), runs ONE agent-scope acquire (it invalidates the CU's L1; the launch's
// workgroups are not held to one per CU, so sc1 loads alone match no row of that table), waits
// for it, and the workgroup passes a barrier before its first plain load of R. Called by every
// thread of every workgroup of the launch, the publisher included (w < 0: no share, but it
// arrives and waits, because it reduces the partials). False: the wait ran out (the launch's
// workgroups were not all resident); *abort is set and the caller stores nothing.
// The counters are not reset here: the next launch counts on the other ticket, which workgroup 0
// of this one zeroes (every user of that one has retired: launches of a stream run in order).
// ------------------------------------------------------------------------------------------
constexpr uint64_t kHeadWaitTicks = 100000000ull;   // s_memrealtime runs at 100 MHz: one second
__device__ inline bool fin_head_run(const FinHead& h, int64_t w, int64_t nw) {
  __shared__ int head_ok;
  if (blockIdx.x == 0 && threadIdx.x <= kTicketShards && h.ticket_next != nullptr)
    __hip_atomic_store(h.ticket_next + threadIdx.x * kTicketStride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int64_t nvb = h.nvb;   // launch_finalize_residual's grid (finalize_blocks)
  if (w >= 0 && w < nvb) {
    Red rd{h.part, nullptr, nullptr};
    rd.parts_only = 1;
    const FinSrc<double> f{h.P, h.B, {h.R0, h.R1, nullptr}, h.cx, h.ml, h.cn, h.S, h.S0, h.chain};
    const double cm = h.cx != nullptr ? pending_max(h.cmax, h.cmax_parts, h.cmax_np, h.cmax_nv) : 0.0;
    for (int64_t vb = w; vb < nvb; vb += nw) {
      double v[4] = {0.0, 0.0, 0.0, 0.0};
      double cxv[kCountAhead];
      fin_block_elems<double, 2, 1, true>(f, vb, nvb, true, false, cxv, v);
      if (h.cx != nullptr) v[3] = count_above(h.cx, h.cn, cxv, vb * 256 + threadIdx.x, nvb * 256, cm);
      grid_reduce<4, 0u, 4, true>(v, rd, (int)vb);
      __syncthreads();   // grid_reduce's LDS row is rewritten by the next block
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned ng = gridDim.x;
    const unsigned sh = blockIdx.x & (kTicketShards - 1);
    const unsigned nsh = ng < (unsigned)kTicketShards ? ng : (unsigned)kTicketShards;
    const unsigned cnt = (ng - sh + kTicketShards - 1) / kTicketShards;
    const unsigned prev = __hip_atomic_fetch_add(h.ticket + (1 + sh) * kTicketStride, 1u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    if (prev == cnt - 1) __hip_atomic_fetch_add(h.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    int ok = 1;
    while (__hip_atomic_load(h.ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != nsh) {
      __builtin_amdgcn_s_sleep(2);
      if (__builtin_amdgcn_s_memrealtime() - t0 > kHeadWaitTicks) {
        ok = 0;
        break;
      }
    }
    if (ok) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      __hip_atomic_store(h.abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    head_ok = ok;
  }
  __syncthreads();
  return head_ok != 0;
}

// ProxGD's line-search trial fused into A^T R (WL 0, one K split): once the block's LDS
// reduction leaves each wave w the 16 gradient rows e == w of its panel — lane (i, q) holding
// columns i and 16 + i of 4 rows, exactly the 16-lanes-per-row layout of k_prox_pgd — every
// wave writes its rows of G and runs the trial on them (prox_pgd_row, the same arithmetic as
// k_prox_pgd) with x = the thresholded iterate; the six trial sums are reduced over the grid.
// HEAD (round 8; f64, WL 0, one K split): the launch first runs the residual finalize that produces
// R (fin_head_run), between its ring's first A loads and its first load of R.
template <typename T, int NT, int PF, bool NTL, bool SPLIT, int WL, bool HEAD>
__device__ __forceinline__ void atr_prox_body(const T* __restrict__ A, typename AtrRPtr<T, HEAD>::type R,
                                              T* __restrict__ G, int64_t m, int64_t n,
                                              const T* __restrict__ x, T* __restrict__ p,
                                              T* __restrict__ pthr, T* __restrict__ z,
                                              double t_, double tmu_, double thres_, const Red& red,
                                              const Pub& pub, int S, T* __restrict__ Gp,
                                              unsigned* __restrict__ pcnt,
                                              unsigned* __restrict__ zf, int keep_mib, const FinHead& fh) {
  // Cancelled by a device-side decision (solver.cpp dc_run): nothing is computed or stored, no
  // counter or ticket is touched. (Testing the flag after the main loop instead measured no
  // faster and would spend a whole pass per cancelled launch.) The decision record still goes
  // to the host: the cancelling decision's own.
  GLX_CLK(0);
  if (red_skipped(red)) {
    if (pub.host != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
      publish_packet(pub.s, pub.ns, pub.host, pub.host_seq, pub.seq);
    return;
  }
  // the extra workgroup (n / 64 * S + 1 in all); with K splits only the panel owners and the
  // publisher reduce (nparts)
  const int nparts = SPLIT ? (int)(n / 64) + (pub.host ? 1 : 0) : -1;
  constexpr int NW = atr_waves<WL>();
  if constexpr (HEAD) {   // the publisher reduces the head's partials: it waits for them too
    static_assert(!SPLIT && WL == 0 && sizeof(T) == 8, "the finalize head: f64, WL 0, one K split");
    if (pub.host != nullptr && blockIdx.x == 0 && !fin_head_run(fh, -1, 0)) return;
  }
  if (publisher_first<6, 0x8u, NW>(pub, red, nparts)) return;
  typedef MF<T> M;
  constexpr int L = 16 * NT;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i = lane & 15;
  typename M::acc_t acc[4][NT];
  const int64_t bid = (int64_t)blockIdx.x - (pub.host ? 1 : 0);
  const int64_t panel = SPLIT ? bid / S : bid, split = SPLIT ? bid % S : 0;
  // Round 4: the row results are stored after the trial sums have been handed to grid_reduce,
  // whose vmcnt(0) drain then waits for six partials instead of wave 0's G / p / p_thr / z stores
  // (the fused epilogue took 8-10 us of the kernel at NS and C2, profiles/r4_clk). Loading the
  // iterate rows before the main loop instead of after it measured 4-5 us slower at NS (+18
  // VGPRs live through the ring, profiles/r4_ab2).
  int64_t col0;
  if constexpr (HEAD) {
    col0 = atr_panel<T, NT, PF, WL, NTL>(A, R, m, n, 1, acc, panel, split, keep_mib,
                                         [&]() { return fin_head_run(fh, bid, n / 64); });
    if (col0 < 0) return;   // the head's wait ran out (uniform over the workgroup)
  } else {
    col0 = atr_panel<T, NT, PF, WL, NTL>(A, R, m, n, SPLIT ? S : 1, acc, panel, split, keep_mib);
  }
  GLX_CLK(4);
  T xa[4][NT];
#pragma unroll
  for (int e = 0; e < atr_ne<WL>(); ++e) {
    if (e != wave) continue;   // wave w owns the rows e == w (4 per lane group)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = col0 + atr_col<T>(M::row(lane, r), e);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) xa[r][nt] = x[row * L + nt * 16 + i];
    }
  }
  double accr[6] = {0.0, 0.0, 0.0, -__builtin_inf(), 0.0, 0.0};
  int slot = work_slot(pub);
  if constexpr (SPLIT) {   // a separate instantiation: the S = 1 kernel keeps 2 blocks per CU
    if (!atr_split_combine<T, NT>(acc, Gp, n, S, panel, split, pcnt, &slot)) return;
  }
  const T t = (T)t_, tmu = (T)tmu_, thres = (T)thres_;
  T gs[4][NT], ps[4][NT], pts[4][NT], zs[4][NT];
  unsigned rows_e[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < atr_ne<WL>(); ++e) {
    if (e != wave) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bool ok[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        gs[r][nt] = acc[e][nt][r];
        ok[nt] = true;
      }
      rows_e[r] = prox_pgd_row<T, 16, NT>(xa[r], gs[r], ok, true, i, t, tmu, thres, ps[r], pts[r], zs[r],
                                          accr, zf != nullptr);
    }
  }
  GLX_CLK(5);
  grid_reduce<6, 0x8u, NW>(accr, red, slot, nparts);
  __shared__ unsigned msk[64];   // the panel's row masks of e (column bitmaps, zf_store_panel)
#pragma unroll
  for (int e = 0; e < atr_ne<WL>(); ++e) {
    if (e != wave) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = col0 + atr_col<T>(M::row(lane, r), e);
      if (zf != nullptr && i == 0) {
        zf[row] = rows_e[r];
        msk[row - col0] = rows_e[r];
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        G[row * L + nt * 16 + i] = gs[r][nt];
        p[row * L + nt * 16 + i] = ps[r][nt];
        pthr[row * L + nt * 16 + i] = pts[r][nt];
        z[row * L + nt * 16 + i] = zs[r][nt];
      }
    }
  }
  if (zf != nullptr) {
    __syncthreads();
    zf_store_panel<atr_pw<WL>()>(msk, zf, n, L, col0);
  }
  GLX_CLK(3);
}

template <typename T, int NT, int PF, bool NTL, bool SPLIT, int WL>
__global__ __launch_bounds__(atr_waves<WL>() * 64, ((WL == 0 || WL == 3) && sizeof(T) == 8) ? 2 : 1) void k_atr_prox(const T* __restrict__ A, const T* __restrict__ R,
                                                  T* __restrict__ G, int64_t m, int64_t n,
                                                  const T* __restrict__ x, T* __restrict__ p,
                                                  T* __restrict__ pthr, T* __restrict__ z,
                                                  double t_, double tmu_, double thres_, Red red,
                                                  Pub pub, int S, T* __restrict__ Gp,
                                                  unsigned* __restrict__ pcnt,
                                                  unsigned* __restrict__ zf, int keep_mib) {
  atr_prox_body<T, NT, PF, NTL, SPLIT, WL, false>(A, R, G, m, n, x, p, pthr, z, t_, tmu_, thres_, red, pub, S, Gp,
                                                  pcnt, zf, keep_mib, FinHead{});
}
// k_atr_prox with the finalize head (f64, WL 0, one K split). R is what the head writes: not
// __restrict__, and no load of it is issued before the head's barrier.
template <int NT, int PF, bool NTL>
__global__ __launch_bounds__(256, 2) void k_atr_prox_head(const double* __restrict__ A, const double* R,
                                                  double* __restrict__ G, int64_t m, int64_t n,
                                                  const double* __restrict__ x, double* __restrict__ p,
                                                  double* __restrict__ pthr, double* __restrict__ z,
                                                  double t_, double tmu_, double thres_, Red red,
                                                  Pub pub, unsigned* __restrict__ zf, int keep_mib,
                                                  FinHead fh) {
  atr_prox_body<double, NT, PF, NTL, false, 0, true>(A, R, G, m, n, x, p, pthr, z, t_, tmu_, thres_, red, pub, 1,
                                                     nullptr, nullptr, zf, keep_mib, fh);
}

// FISTA's backtracking trial fused into A^T R the same way (WL 0, one K split): each wave runs
// fista_row (the arithmetic of k_fista_trial) on its 16 gradient rows, with y the extrapolated
// point and xk the current iterate; writes G, xc, v_next, y_next and reduces the four sums.
template <typename T, int NT, int PF, bool NTL, bool SPLIT, int WL>
__global__ __launch_bounds__(atr_waves<WL>() * 64, ((WL == 0 || WL == 3) && sizeof(T) == 8) ? 2 : 1) void k_atr_fista(const T* __restrict__ A, const T* __restrict__ R,
                                                   T* __restrict__ G, int64_t m, int64_t n,
                                                   const T* __restrict__ y, const T* __restrict__ xk,
                                                   T* __restrict__ xc, T* __restrict__ vnext,
                                                   T* __restrict__ ynext, double t_, double tmu_,
                                                   double thres_, double theta_, double a1_,
                                                   double b1_, Red red, Pub pub, int S,
                                                   T* __restrict__ Gp, unsigned* __restrict__ pcnt,
                                                   T* __restrict__ ec, unsigned* __restrict__ zf,
                                                   int keep_mib) {
  if (red_skipped(red)) {   // cancelled by a device-side decision (as k_atr_prox)
    if (pub.host != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
      publish_packet(pub.s, pub.ns, pub.host, pub.host_seq, pub.seq);
    return;
  }
  const int nparts = SPLIT ? (int)(n / 64) + (pub.host ? 1 : 0) : -1;   // see k_atr_prox
  constexpr int NW = atr_waves<WL>();
  if (publisher_first<4, 0x8u, NW>(pub, red, nparts)) return;
  typedef MF<T> M;
  constexpr int L = 16 * NT;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i = lane & 15;
  typename M::acc_t acc[4][NT];
  const int64_t bid = (int64_t)blockIdx.x - (pub.host ? 1 : 0);
  const int64_t panel = SPLIT ? bid / S : bid, split = SPLIT ? bid % S : 0;
  const int64_t col0 = atr_panel<T, NT, PF, WL, NTL>(A, R, m, n, SPLIT ? S : 1, acc, panel, split, keep_mib);
  double accr[4] = {0.0, 0.0, 0.0, -__builtin_inf()};
  int slot = work_slot(pub);
  if constexpr (SPLIT) {   // fixed reduction slots, see atr_split_combine
    if (!atr_split_combine<T, NT>(acc, Gp, n, S, panel, split, pcnt, &slot)) return;
  }
  const T t = (T)t_, tmu = (T)tmu_, thres = (T)thres_, theta = (T)theta_, a1 = (T)a1_, b1 = (T)b1_;
  __shared__ unsigned msk[64];   // the panel's row masks of e_c (column bitmaps, zf_store_panel)
#pragma unroll
  for (int e = 0; e < atr_ne<WL>(); ++e) {
    if (e != wave) continue;   // wave w owns the rows e == w
    T ya[4][NT], xa[4][NT];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = col0 + atr_col<T>(M::row(lane, r), e);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        ya[r][nt] = y[row * L + nt * 16 + i];
        xa[r][nt] = xk[row * L + nt * 16 + i];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = col0 + atr_col<T>(M::row(lane, r), e);
      T gv[NT], xcv[NT], vnv[NT], ynv[NT], ecv[NT];
      bool ok[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        gv[nt] = acc[e][nt][r];
        ok[nt] = true;
        G[row * L + nt * 16 + i] = gv[nt];
      }
      const unsigned rowe = fista_row<T, 16, NT, true>(ya[r], gv, xa[r], ok, true, i, t, tmu, thres, theta,
                                                   a1, b1, T(0), T(0), xcv, vnv, ynv, accr,
                                                   ec != nullptr ? ecv : nullptr);
      if (zf != nullptr && i == 0) {
        zf[row] = rowe;
        msk[row - col0] = rowe;
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        xc[row * L + nt * 16 + i] = xcv[nt];
        vnext[row * L + nt * 16 + i] = vnv[nt];
        ynext[row * L + nt * 16 + i] = ynv[nt];
        if (ec != nullptr) ec[row * L + nt * 16 + i] = ecv[nt];
      }
    }
  }
  grid_reduce<4, 0x8u, NW>(accr, red, slot, nparts);
  if (zf != nullptr) {   // (grid_reduce's barriers ordered the msk stores above)
    __syncthreads();
    zf_store_panel<atr_pw<WL>()>(msk, zf, n, L, col0);
  }
}

// ------------------------------------------------------------------------------------------
// The "rows after the product" epilogues (dual ADMM's row step, the certificate's row terms, dual
// ALM's inner step). Each is a policy Epi, a struct of pointers and scalars with
//   kIterate                                  the frame loads the wave's rows of Epi::x into xa
//   rows<NT, WL>(xa, gs, col0, slot, nparts)  the row arithmetic on the panel layout an A^T R
//                                             epilogue holds: wave w < NE owns the 16 rows e == w
//                                             of the panel at col0, lane (i, q) holding columns i
//                                             (and 16 + i) of 4 of them; gs = those values of the
//                                             product. Called by every thread of the workgroup.
// and runs under two frames: atr_rows_body at the end of the product (the k_atr_* kernels) and
// panel_rows_body on the slabs launch_atr wrote under the same plan (the k_*_panel kernels). One
// rows() serves both, so the fused and the unfused form write the same bits, sums included.
// rows() hands the policy's pointers to a static run(): __restrict__ tells the compiler something
// only on a function's parameters, and without it the row stores are scheduled as if they could
// alias (k_admm_dual_panel's NT 2 form grew by 60 instructions).
// The kernels hand their policy over by reference: how a packet reaches a body decides whether
// the kernel gets a scratch frame (round 8, k_atr_prox).
// ------------------------------------------------------------------------------------------
// The frame fused into the product: once the block's reduction (and, with K splits, the last
// arriver's slab combine) leaves each wave its 16 complete rows, Epi::rows runs on them. No
// packet, no masks. The iterate's rows are loaded before the combine, not after it.
template <typename T, int NT, int PF, bool NTL, bool SPLIT, int WL, typename Epi>
__device__ __forceinline__ void atr_rows_body(const T* __restrict__ A, const T* __restrict__ R, int64_t m,
                                              int64_t n, int S, T* __restrict__ Gp,
                                              unsigned* __restrict__ pcnt, int keep_mib, const Epi& epi) {
  const int nparts = SPLIT ? (int)(n / 64) : -1;   // with K splits only the panel owners reduce
  typedef MF<T> M;
  constexpr int L = 16 * NT;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i = lane & 15;
  typename M::acc_t acc[4][NT];
  const int64_t bid = (int64_t)blockIdx.x;
  const int64_t panel = SPLIT ? bid / S : bid, split = SPLIT ? bid % S : 0;
  const int64_t col0 = atr_panel<T, NT, PF, WL, NTL>(A, R, m, n, SPLIT ? S : 1, acc, panel, split, keep_mib);
  T xa[4][NT], gs[4][NT];
  if constexpr (Epi::kIterate) {
#pragma unroll
    for (int e = 0; e < atr_ne<WL>(); ++e) {
      if (e != wave) continue;   // wave w owns the rows e == w (4 per lane group)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = col0 + atr_col<T>(M::row(lane, r), e);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) xa[r][nt] = epi.x[row * L + nt * 16 + i];
      }
    }
  }
  int slot = (int)blockIdx.x;
  if constexpr (SPLIT) {   // fixed reduction slots, see atr_split_combine
    if (!atr_split_combine<T, NT>(acc, Gp, n, S, panel, split, pcnt, &slot)) return;
  }
#pragma unroll
  for (int e = 0; e < atr_ne<WL>(); ++e) {
    if (e != wave) continue;   // (static register index into acc)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) gs[r][nt] = acc[e][nt][r];
  }
  epi.template rows<NT, WL>(xa, gs, col0, slot, nparts);
}

// The unfused frame on the same layout: the product = the sum, in slab order (atr_split_combine's
// order), of the S slabs of g; one workgroup per panel, slot = panel.
template <typename T, int NT, int WL, typename Epi>
__device__ __forceinline__ void panel_rows_body(const T* __restrict__ g, int S, int64_t n, const Epi& epi) {
  typedef MF<T> M;
  constexpr int L = 16 * NT;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i = lane & 15;
  const int64_t col0 = (int64_t)blockIdx.x * atr_pw<WL>();
  const int64_t nl = n * L;
  T xa[4][NT], gs[4][NT];
  if (wave < atr_ne<WL>()) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = col0 + atr_col<T>(M::row(lane, r), wave);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if constexpr (Epi::kIterate) xa[r][nt] = epi.x[row * L + nt * 16 + i];
        gs[r][nt] = slab_sum(g, S, nl, row * L + nt * 16 + i);
      }
    }
  }
  epi.template rows<NT, WL>(xa, gs, col0, (int)blockIdx.x, -1);
}

// Dual ADMM's row step (gl_ADMM_dual.py:64-67): xa = the wave's values of the iterate, gs of
// g = A^T z. Runs admm_dual_row (the arithmetic of k_admm_dual, kernels_admm.hip), hands the two
// sums [sum_i ||x+_i||, max |x+|] to grid_reduce and then stores G (when non-null), u+, x+ and r,
// as k_atr_prox orders them (waves past NE reduce identities).
template <typename T>
struct AdmmRows {
  static constexpr bool kIterate = true;
  const T* x;
  T *G, *un, *xn, *rn;
  T rho, taurho, mu;
  const Red& red;
  template <int NT, int WL>
  __device__ __forceinline__ void rows(const T (&xa)[4][NT], const T (&gs)[4][NT], int64_t col0, int slot,
                                       int nparts) const {
    run<NT, WL>(xa, gs, col0, G, un, xn, rn, rho, taurho, mu, red, slot, nparts);
  }
  template <int NT, int WL>
  static __device__ inline void run(const T (&xa)[4][NT], const T (&gs)[4][NT], int64_t col0,
                                    T* __restrict__ G, T* __restrict__ un, T* __restrict__ xn,
                                    T* __restrict__ rn, T rho, T taurho, T mu, const Red& red, int slot,
                                    int nparts) {
    typedef MF<T> M;
    constexpr int L = 16 * NT;
    constexpr int NW = atr_waves<WL>();
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i = lane & 15;
    const bool mine = wave < atr_ne<WL>();
    double accr[2] = {0.0, -__builtin_inf()};
    T us[4][NT], xs[4][NT], rs[4][NT];
    if (mine) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bool ok[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) ok[nt] = true;
        admm_dual_row<T, 16, NT>(xa[r], gs[r], ok, true, i, rho, taurho, mu, us[r], xs[r], rs[r], accr);
      }
    }
    grid_reduce<2, 0x2u, NW>(accr, red, slot, nparts);
    if (!mine) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = col0 + atr_col<T>(M::row(lane, r), wave);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        if (G != nullptr) G[row * L + nt * 16 + i] = gs[r][nt];
        un[row * L + nt * 16 + i] = us[r][nt];
        xn[row * L + nt * 16 + i] = xs[r][nt];
        rn[row * L + nt * 16 + i] = rs[r][nt];
      }
    }
  }
};

template <typename T, int NT, int PF, bool NTL, bool SPLIT, int WL>
__global__ __launch_bounds__(atr_waves<WL>() * 64, ((WL == 0 || WL == 3) && sizeof(T) == 8) ? 2 : 1) void k_atr_admm(const T* __restrict__ A, const T* __restrict__ Z,
                                                  T* __restrict__ G, int64_t m, int64_t n,
                                                  const T* __restrict__ x, T* __restrict__ un,
                                                  T* __restrict__ xn, T* __restrict__ rn,
                                                  double rho_, double taurho_, double mu_, Red red,
                                                  int S, T* __restrict__ Gp,
                                                  unsigned* __restrict__ pcnt, int keep_mib) {
  const AdmmRows<T> epi{x, G, un, xn, rn, (T)rho_, (T)taurho_, (T)mu_, red};
  atr_rows_body<T, NT, PF, NTL, SPLIT, WL>(A, Z, m, n, S, Gp, pcnt, keep_mib, epi);
}
template <typename T, int NT, int WL>
__global__ __launch_bounds__(atr_waves<WL>() * 64) void k_admm_dual_panel(const T* __restrict__ x, const T* __restrict__ g, int S,
                                                  T* __restrict__ gout, T* __restrict__ un,
                                                  T* __restrict__ xn, T* __restrict__ rn, int64_t n,
                                                  double rho_, double taurho_, double mu_, Red red) {
  const AdmmRows<T> epi{x, gout, un, xn, rn, (T)rho_, (T)taurho_, (T)mu_, red};
  panel_rows_body<T, NT, WL>(g, S, n, epi);
}

// The certificate's row terms: xa = the wave's values of the iterate, gs of g = A^T r. Runs
// cert_row, hands its five sums to grid_reduce and then stores G (only where the caller asks for
// it) and the rows' ||g_i|| as doubles (rn, when non-null). Waves past NE reduce identities.
template <typename T>
struct CertRows {
  static constexpr bool kIterate = true;
  const T* x;
  T* G;
  double* rn;
  T mu;
  const Red& red;
  template <int NT, int WL>
  __device__ __forceinline__ void rows(const T (&xa)[4][NT], const T (&gs)[4][NT], int64_t col0, int slot,
                                       int nparts) const {
    run<NT, WL>(xa, gs, col0, G, rn, mu, red, slot, nparts);
  }
  template <int NT, int WL>
  static __device__ inline void run(const T (&xa)[4][NT], const T (&gs)[4][NT], int64_t col0,
                                    T* __restrict__ G, double* __restrict__ rn, T mu, const Red& red,
                                    int slot, int nparts) {
    typedef MF<T> M;
    constexpr int L = 16 * NT;
    constexpr int NW = atr_waves<WL>();
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i = lane & 15;
    const bool mine = wave < atr_ne<WL>();
    double accr[5] = {0.0, -__builtin_inf(), -__builtin_inf(), 0.0, 0.0};
    T gn[4];
    if (mine) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bool ok[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) ok[nt] = true;
        gn[r] = cert_row<T, 16, NT>(xa[r], gs[r], ok, true, i, mu, accr);
      }
    }
    grid_reduce<5, 0x6u, NW>(accr, red, slot, nparts);
    if (!mine) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = col0 + atr_col<T>(M::row(lane, r), wave);
      if (G != nullptr) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) G[row * L + nt * 16 + i] = gs[r][nt];
      }
      if (rn != nullptr && i == 0) rn[row] = (double)gn[r];
    }
  }
};

template <typename T, int NT, int PF, bool NTL, bool SPLIT, int WL>
__global__ __launch_bounds__(atr_waves<WL>() * 64, ((WL == 0 || WL == 3) && sizeof(T) == 8) ? 2 : 1) void k_atr_cert(const T* __restrict__ A, const T* __restrict__ R,
                                                  T* __restrict__ G, int64_t m, int64_t n,
                                                  const T* __restrict__ x, double* __restrict__ rn,
                                                  double mu_, Red red, int S, T* __restrict__ Gp,
                                                  unsigned* __restrict__ pcnt, int keep_mib) {
  const CertRows<T> epi{x, G, rn, (T)mu_, red};
  atr_rows_body<T, NT, PF, NTL, SPLIT, WL>(A, R, m, n, S, Gp, pcnt, keep_mib, epi);
}
template <typename T, int NT, int WL>
__global__ __launch_bounds__(atr_waves<WL>() * 64) void k_cert_panel(const T* __restrict__ x, const T* __restrict__ g, int S,
                                                  T* __restrict__ gout, double* __restrict__ rn,
                                                  int64_t n, double mu_, Red red) {
  const CertRows<T> epi{x, gout, rn, (T)mu_, red};
  panel_rows_body<T, NT, WL>(g, S, n, epi);
}

// One step of dual ALM's inner loop (gl_ALM_dual.py:56-61), A = Qn (n x n, symmetric) and R = y:
// ps = the wave's 16 complete rows of P = Qn y. Reads y, J and u itself, runs alm_inner_row and
// stores u+ (un; may be u itself: a row's lanes read their own elements before they write them)
// and, where yn != NULL, y+. yn is never the y the product reads: other workgroups may still be
// streaming it. No iterate, no sums, so no grid reduction and no slot; waves past NE have no rows.
template <typename T>
struct AlmScalars {
  T t, mu, gamma, a1, gn;
};
template <typename T>
struct AlmRows {
  static constexpr bool kIterate = false;
  const T *y, *J, *u;
  T *un, *yn;
  const AlmScalars<T>& sc;
  template <int NT, int WL>
  __device__ __forceinline__ void rows(const T (&)[4][NT], const T (&ps)[4][NT], int64_t col0, int, int) const {
    run<NT, WL>(ps, col0, y, J, u, un, yn, sc);
  }
  template <int NT, int WL>
  static __device__ inline void run(const T (&ps)[4][NT], int64_t col0, const T* __restrict__ y,
                                    const T* __restrict__ J, const T* u, T* un, T* __restrict__ yn,
                                    const AlmScalars<T>& sc) {
    typedef MF<T> M;
    constexpr int L = 16 * NT;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int i = lane & 15;
    if (wave >= atr_ne<WL>()) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = col0 + atr_col<T>(M::row(lane, r), wave);
      T yv[NT], jv[NT], uv[NT], uo[NT], yo[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        yv[nt] = y[row * L + nt * 16 + i];
        jv[nt] = J[row * L + nt * 16 + i];
        uv[nt] = u[row * L + nt * 16 + i];
      }
      alm_inner_row<T, 16, NT>(ps[r], yv, jv, uv, sc.t, sc.mu, sc.gamma, sc.a1, sc.gn, uo, yo);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        un[row * L + nt * 16 + i] = uo[nt];
        if (yn != nullptr) yn[row * L + nt * 16 + i] = yo[nt];
      }
    }
  }
};

// The inner step fused into P = Qn^T y (= Qn y): one launch per inner step.
template <typename T, int NT, int PF, bool NTL, bool SPLIT, int WL>
__global__ __launch_bounds__(atr_waves<WL>() * 64, ((WL == 0 || WL == 3) && sizeof(T) == 8) ? 2 : 1) void k_atr_alm(const T* __restrict__ Qn, const T* __restrict__ y,
                                                  int64_t n, const T* __restrict__ J, const T* u, T* un,
                                                  T* __restrict__ yn, AlmScalars<T> sc, int S,
                                                  T* __restrict__ Gp, unsigned* __restrict__ pcnt,
                                                  int keep_mib) {
  const AlmRows<T> epi{y, J, u, un, yn, sc};
  atr_rows_body<T, NT, PF, NTL, SPLIT, WL>(Qn, y, n, n, S, Gp, pcnt, keep_mib, epi);
}
template <typename T, int NT, int WL>
__global__ __launch_bounds__(atr_waves<WL>() * 64) void k_alm_inner_panel(const T* __restrict__ P, int S, int64_t n,
                                                  const T* __restrict__ y, const T* __restrict__ J,
                                                  const T* u, T* un, T* __restrict__ yn,
                                                  AlmScalars<T> sc) {
  const AlmRows<T> epi{y, J, u, un, yn, sc};
  panel_rows_body<T, NT, WL>(P, S, n, epi);
}


// A^T R on VALU: a thread owns E consecutive columns of A over a row range; R[row][c0..c0+LB)
// is wave-uniform (scalar loads). Gp[blockIdx.y][n][l].
template <typename T, int LB, bool VEC>
__global__ __launch_bounds__(256) void k_atr_valu(const T* __restrict__ A, const T* __restrict__ R,
                                                  T* __restrict__ Gp, int64_t m, int64_t n,
                                                  int64_t l, int c0, int S) {
  constexpr int E = VEC ? (16 / (int)sizeof(T)) : 1;
  const int64_t col = ((int64_t)blockIdx.x * 256 + threadIdx.x) * E;
  const int s = blockIdx.y;
  const int64_t rb = m * s / S, re = m * (s + 1) / S;
  const int nc = (int)((l - c0) < LB ? (l - c0) : LB);
  const bool active = col < n;
  const int64_t ccol = active ? col : 0;

  T acc[E][LB];
#pragma unroll
  for (int e = 0; e < E; ++e)
#pragma unroll
    for (int c = 0; c < LB; ++c) acc[e][c] = T(0);

  const T* ap = A + rb * n + ccol;
  const T* rp = R + rb * l + c0;
#pragma unroll 4
  for (int64_t row = rb; row < re; ++row) {
    T a[E];
    if constexpr (VEC) {
      typedef typename MF<T>::vec_t V;
      const V v = *reinterpret_cast<const V*>(ap);
#pragma unroll
      for (int e = 0; e < E; ++e) a[e] = v[e];
    } else {
      a[0] = *ap;
    }
    T rv[LB];
#pragma unroll
    for (int c = 0; c < LB; ++c) rv[c] = (c < nc) ? rp[c] : T(0);
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
      for (int c = 0; c < LB; ++c) acc[e][c] = __builtin_fma(a[e], rv[c], acc[e][c]);
    ap += n;
    rp += l;
  }
  if (!active) return;
  T* gout = Gp + (int64_t)s * n * l;
#pragma unroll
  for (int e = 0; e < E; ++e)
#pragma unroll
    for (int c = 0; c < LB; ++c)
      if (c < nc) gout[(col + e) * l + c0 + c] = acc[e][c];
}


template <typename T, int LB>
static void atr_valu_lb(const GemmPlan& p, const T* A, const T* R, T* Gp, hipStream_t st) {
  constexpr int E = 16 / sizeof(T);
  const int64_t cols_per_block = 256 * (p.atr_vec ? E : 1);
  const dim3 grid((unsigned)cdiv(p.n, cols_per_block), (unsigned)p.atr_S);
  for (int64_t c0 = 0; c0 < p.l; c0 += LB) {
    if (p.atr_vec)
      glx_launch((k_atr_valu<T, LB, true>), grid, dim3(256), 0, st, A, R, Gp, p.m, p.n,
                         p.l, (int)c0, p.atr_S);
    else
      glx_launch((k_atr_valu<T, LB, false>), grid, dim3(256), 0, st, A, R, Gp, p.m, p.n,
                         p.l, (int)c0, p.atr_S);
  }
}

template <typename T, int NT, int PF, int WL, bool NTL>
static void atr_mfma_go(const GemmPlan& p, const T* A, const T* R, T* Gp, hipStream_t st) {
  const dim3 grid((unsigned)(p.n / (WL == 1 ? 256 : atr_pw<WL>())), (unsigned)p.atr_S);
  static const size_t pad = lds_pad(k_atr_mfma<T, NT, PF, WL, NTL>, "GLX_ATR_LDS_PAD");
  glx_launch((k_atr_mfma<T, NT, PF, WL, NTL>), grid, dim3(atr_waves<WL>() * 64), pad, st, A, R, Gp, p.m, p.n, p.atr_S,
             p.atr_keep_mib);
}

// The tile visitor of the three A^T R launchers: f(index of the plan's tile in kAtrTiles, NT) as
// compile-time constants, if its kernels (FUSED: k_atr_prox / k_atr_fista) are built for T.
template <typename T, bool FUSED, typename F>
static void atr_visit(const GemmPlan& p, const char* what, F&& f) {
  bool built = false;
  with_const<1, 2>((int)(p.l / 16), [&](auto nt) {
    visit_tile(kAtrTiles, p.atr, [&](auto i) {
      constexpr const AtrTile& t = kAtrTiles[decltype(i)::value];
      if constexpr (t.fam == Fam::Mfma && ((FUSED ? t.fused : t.dtypes) & dtype_bit(sizeof(T))) != 0) {
        f(i, nt);
        built = true;
      }
    });
  });
  if (!built && !FUSED && p.atr->wl == 3) throw Error{GLX_E_INVALID, "A^T R: the 32-column panel is f64"};
  if (!built)
    throw Error{GLX_E_INVALID, std::string(what) + ": tile WL" + std::to_string(p.atr->wl) + " PF" +
                                   std::to_string(p.atr->pf) + " NTL" + std::to_string((int)p.atr->ntl) +
                                   " is not built (round 6 pruning)"};
}

template <typename T>
void launch_atr(const GemmPlan& p, const T* A, const T* R, T* Gp, hipStream_t st) {
  if (p.atr->fam == Fam::Valu) {
    with_const<1, 2, 4, 8>(p.atr_lb, [&](auto lb) { atr_valu_lb<T, decltype(lb)::value>(p, A, R, Gp, st); });
    return;
  }
  atr_visit<T, false>(p, "A^T R", [&](auto i, auto nt) {
    constexpr const AtrTile& t = kAtrTiles[decltype(i)::value];
    atr_mfma_go<T, decltype(nt)::value, t.pf, t.wl, t.ntl>(p, A, R, Gp, st);
  });
}

// The template arguments of a fused A^T R kernel after T, as one type a generic lambda reads.
template <int NT_, int PF_, bool NTL_, bool SPLIT_, int WL_>
struct AtrArgs {
  static constexpr int NT = NT_, PF = PF_, WL = WL_;
  static constexpr bool NTL = NTL_, SPLIT = SPLIT_;
};

// The one launcher of the fused A^T R families. kernel_of(AtrArgs) names the family's kernel at
// those arguments; go(AtrArgs, kernel, grid, block, pad, S) makes the launch with its own argument
// list. The grid is a 1-D n / panel * S workgroups (+ `extra`: the publisher's). With K splits on a
// 64-column panel the SPLIT kernel runs without an occupancy pad; otherwise the plain one (the S = 1
// kernel keeps 2 blocks per CU) with S = 1. The planner never splits K on the 32-column panel
// (fuses(), planner.cpp), so no SPLIT kernel is built for it.
template <typename T, typename KernelOf, typename Go>
static void atr_fused_launch(const GemmPlan& p, const char* what, int extra, const T* Gp, const unsigned* pcnt,
                             KernelOf kernel_of, Go&& go) {
  if (p.atr_S > 1 && (Gp == nullptr || pcnt == nullptr))
    throw Error{GLX_E_INVALID, "fused A^T R with K splits needs slab and counter buffers"};
  atr_visit<T, true>(p, what, [&](auto i, auto nt) {
    constexpr const AtrTile& tile = kAtrTiles[decltype(i)::value];
    constexpr int NT = decltype(nt)::value, WL = tile.wl;
    const dim3 grid((unsigned)(p.n / atr_pw<WL>() * p.atr_S + extra));
    const dim3 block(atr_waves<WL>() * 64);
    if constexpr (WL != 3 && WL != 4) {
      if (p.atr_S > 1) {
        const AtrArgs<NT, tile.pf, tile.ntl, true, WL> a;
        go(a, kernel_of(a), grid, block, (size_t)0, p.atr_S);
        return;
      }
    }
    const AtrArgs<NT, tile.pf, tile.ntl, false, WL> a;
    static const size_t pad = lds_pad(kernel_of(a), "GLX_ATR_LDS_PAD");
    go(a, kernel_of(a), grid, block, pad, 1);
  });
}

// The launcher of the unfused twins: go(NT, WL, grid, block), one workgroup per panel.
template <typename T, typename Go>
static void panel_rows_launch(const GemmPlan& p, const char* what, Go&& go) {
  atr_visit<T, true>(p, what, [&](auto i, auto nt) {
    constexpr int WL = kAtrTiles[decltype(i)::value].wl;
    go(nt, std::integral_constant<int, WL>{}, dim3((unsigned)(p.n / atr_pw<WL>())), dim3(atr_waves<WL>() * 64));
  });
}

template <typename T>
void launch_atr_prox(const GemmPlan& p, const T* A, const T* R, T* G, const T* x, T* pp, T* pthr,
                     T* z, double t, double mu, double thres, Red red, hipStream_t st, Pub pub,
                     T* Gp, unsigned* pcnt, unsigned* zf, const FinHead* head) {
  FinHead hd;
  if (head != nullptr) {
    hd = *head;
    if (hd.S0 <= 0) hd.S0 = hd.S;   // (as launch_finalize_residual)
    if (!atr_prox_head_ok(p, hd.S, hd.S0) || red.skip != nullptr)
      throw Error{GLX_E_INVALID, "fused A^T R + trial: this plan or finalize takes no head"};
    if (!hd.P || !hd.B || !hd.R1 || (const void*)hd.R1 != (const void*)R || !hd.part || !hd.ticket || !hd.abort ||
        hd.ticket_next == hd.ticket || (hd.chain == 0 && !hd.R0) || (hd.cx && !hd.cmax && !hd.cmax_parts))
      throw Error{GLX_E_INVALID, "fused A^T R + trial: bad finalize head"};
    hd.nvb = finalize_blocks(hd.ml, hd.S, hd.chain ? hd.S0 : 0, hd.cx ? hd.cn : 0);
    head = &hd;
  }
  atr_fused_launch<T>(
      p, "fused A^T R + trial", pub.host ? 1 : 0, Gp, pcnt,
      [](auto a) { return &k_atr_prox<T, a.NT, a.PF, a.NTL, a.SPLIT, a.WL>; },
      [&](auto a, auto kernel, dim3 grid, dim3 block, size_t pad, int S) {
        if (head != nullptr) {
          if constexpr (std::is_same<T, double>::value && a.WL == 0) {
            static const size_t hpad = lds_pad(k_atr_prox_head<a.NT, a.PF, a.NTL>, "GLX_ATR_LDS_PAD");
            glx_launch((k_atr_prox_head<a.NT, a.PF, a.NTL>), grid, block, hpad, st, A, R, G, p.m, p.n, x, pp, pthr, z, t,
                       t * mu, thres, red, pub, zf, p.atr_keep_mib, *head);
            return;
          }
          throw Error{GLX_E_INVALID, "fused A^T R + trial: the finalize head is built for the f64 four-wave panel"};
        }
        glx_launch(kernel, grid, block, pad, st, A, R, G, p.m, p.n, x, pp, pthr, z, t, t * mu, thres, red, pub, S, Gp,
                   pcnt, zf, p.atr_keep_mib);
      });
}

template <typename T>
void launch_atr_fista(const GemmPlan& p, const T* A, const T* R, T* G, const T* y, const T* xk,
                      T* xc, T* vn, T* yn, double t, double mu, double thres, double theta,
                      double theta_next, Red red, hipStream_t st, Pub pub, T* Gp, unsigned* pcnt,
                      T* ec, unsigned* zf) {
  atr_fused_launch<T>(
      p, "fused A^T R + FISTA trial", pub.host ? 1 : 0, Gp, pcnt,
      [](auto a) { return &k_atr_fista<T, a.NT, a.PF, a.NTL, a.SPLIT, a.WL>; },
      [&](auto, auto kernel, dim3 grid, dim3 block, size_t pad, int S) {
        glx_launch(kernel, grid, block, pad, st, A, R, G, p.m, p.n, y, xk, xc, vn, yn, t, t * mu, thres, theta,
                   1.0 - theta_next, theta_next, red, pub, S, Gp, pcnt, ec, zf, p.atr_keep_mib);
      });
}

template <typename T>
void launch_atr_admm(const GemmPlan& p, const T* A, const T* Z, T* G, const T* x, T* un, T* xn, T* rn,
                     double rho, double taurho, double mu, Red red, hipStream_t st, T* Gp,
                     unsigned* pcnt) {
  atr_fused_launch<T>(
      p, "fused A^T z + ADMM row step", 0, Gp, pcnt,
      [](auto a) { return &k_atr_admm<T, a.NT, a.PF, a.NTL, a.SPLIT, a.WL>; },
      [&](auto, auto kernel, dim3 grid, dim3 block, size_t pad, int S) {
        glx_launch(kernel, grid, block, pad, st, A, Z, G, p.m, p.n, x, un, xn, rn, rho, taurho, mu, red, S, Gp, pcnt,
                   p.atr_keep_mib);
      });
}
template <typename T>
void launch_admm_dual_panel(const GemmPlan& p, const T* x, const T* g, int S, T* gout, T* un, T* xn,
                            T* rn, double rho, double taurho, double mu, Red red, hipStream_t st) {
  panel_rows_launch<T>(p, "ADMM row step on the panel layout", [&](auto nt, auto wl, dim3 grid, dim3 block) {
    glx_launch((k_admm_dual_panel<T, nt.value, wl.value>), grid, block, 0, st, x, g, S, gout, un, xn, rn, p.n, rho,
               taurho, mu, red);
  });
}

template <typename T>
void launch_atr_cert(const GemmPlan& p, const T* A, const T* R, T* G, const T* x, double* rn, double mu,
                     Red red, hipStream_t st, T* Gp, unsigned* pcnt) {
  atr_fused_launch<T>(
      p, "fused A^T r + certificate rows", 0, Gp, pcnt,
      [](auto a) { return &k_atr_cert<T, a.NT, a.PF, a.NTL, a.SPLIT, a.WL>; },
      [&](auto, auto kernel, dim3 grid, dim3 block, size_t pad, int S) {
        glx_launch(kernel, grid, block, pad, st, A, R, G, p.m, p.n, x, rn, mu, red, S, Gp, pcnt, p.atr_keep_mib);
      });
}
template <typename T>
void launch_cert_panel(const GemmPlan& p, const T* x, const T* g, int S, T* gout, double* rn, double mu,
                       Red red, hipStream_t st) {
  panel_rows_launch<T>(p, "certificate rows on the panel layout", [&](auto nt, auto wl, dim3 grid, dim3 block) {
    glx_launch((k_cert_panel<T, nt.value, wl.value>), grid, block, 0, st, x, g, S, gout, rn, p.n, mu, red);
  });
}

template <typename T>
static AlmScalars<T> alm_scalars(double t, double mu, double gamma, double gamma_next) {
  return AlmScalars<T>{(T)t, (T)mu, (T)gamma, (T)(1.0 - gamma_next), (T)gamma_next};
}
template <typename T>
void launch_atr_alm(const GemmPlan& p, const T* Qn, const T* y, const T* J, const T* u, T* un, T* yn,
                    double t, double mu, double gamma, double gamma_next, hipStream_t st, T* Gp,
                    unsigned* pcnt) {
  if (p.m != p.n) throw Error{GLX_E_INVALID, "fused Qn y: the plan must be of the square (n, n, l)"};
  if (yn == y) throw Error{GLX_E_INVALID, "fused Qn y: y+ must not be written over the product's operand"};
  const AlmScalars<T> sc = alm_scalars<T>(t, mu, gamma, gamma_next);
  atr_fused_launch<T>(
      p, "fused Qn y + ALM inner step", 0, Gp, pcnt,
      [](auto a) { return &k_atr_alm<T, a.NT, a.PF, a.NTL, a.SPLIT, a.WL>; },
      [&](auto, auto kernel, dim3 grid, dim3 block, size_t pad, int S) {
        glx_launch(kernel, grid, block, pad, st, Qn, y, p.n, J, u, un, yn, sc, S, Gp, pcnt, p.atr_keep_mib);
      });
}
template <typename T>
void launch_alm_inner_panel(const GemmPlan& p, const T* P, int S, const T* y, const T* J, const T* u, T* un,
                            T* yn, double t, double mu, double gamma, double gamma_next, hipStream_t st) {
  const AlmScalars<T> sc = alm_scalars<T>(t, mu, gamma, gamma_next);
  panel_rows_launch<T>(p, "ALM inner step on the panel layout", [&](auto nt, auto wl, dim3 grid, dim3 block) {
    glx_launch((k_alm_inner_panel<T, nt.value, wl.value>), grid, block, 0, st, P, S, p.n, y, J, u, un, yn, sc);
  });
}

// (dual ALM is fp64 only)
template void launch_atr_alm<double>(const GemmPlan&, const double*, const double*, const double*,
                                     const double*, double*, double*, double, double, double, double,
                                     hipStream_t, double*, unsigned*);
template void launch_alm_inner_panel<double>(const GemmPlan&, const double*, int, const double*,
                                             const double*, const double*, double*, double*, double,
                                             double, double, double, hipStream_t);
template void launch_admm_dual_panel<double>(const GemmPlan&, const double*, const double*, int, double*,
                                             double*, double*, double*, double, double, double, Red,
                                             hipStream_t);
template void launch_admm_dual_panel<float>(const GemmPlan&, const float*, const float*, int, float*,
                                            float*, float*, float*, double, double, double, Red,
                                            hipStream_t);
template void launch_atr_admm<double>(const GemmPlan&, const double*, const double*, double*,
                                      const double*, double*, double*, double*, double, double,
                                      double, Red, hipStream_t, double*, unsigned*);
template void launch_atr_admm<float>(const GemmPlan&, const float*, const float*, float*,
                                     const float*, float*, float*, float*, double, double, double,
                                     Red, hipStream_t, float*, unsigned*);
template void launch_atr_cert<double>(const GemmPlan&, const double*, const double*, double*,
                                      const double*, double*, double, Red, hipStream_t, double*,
                                      unsigned*);
template void launch_atr_cert<float>(const GemmPlan&, const float*, const float*, float*, const float*,
                                     double*, double, Red, hipStream_t, float*, unsigned*);
template void launch_cert_panel<double>(const GemmPlan&, const double*, const double*, int, double*,
                                        double*, double, Red, hipStream_t);
template void launch_cert_panel<float>(const GemmPlan&, const float*, const float*, int, float*, double*,
                                       double, Red, hipStream_t);
template void launch_atr<double>(const GemmPlan&, const double*, const double*, double*, hipStream_t);
template void launch_atr_fista<double>(const GemmPlan&, const double*, const double*, double*,
                                       const double*, const double*, double*, double*, double*,
                                       double, double, double, double, double, Red, hipStream_t, Pub,
                                       double*, unsigned*, double*, unsigned*);
template void launch_atr_fista<float>(const GemmPlan&, const float*, const float*, float*,
                                      const float*, const float*, float*, float*, float*, double,
                                      double, double, double, double, Red, hipStream_t, Pub,
                                      float*, unsigned*, float*, unsigned*);
template void launch_atr_prox<double>(const GemmPlan&, const double*, const double*, double*,
                                      const double*, double*, double*, double*, double, double,
                                      double, Red, hipStream_t, Pub, double*, unsigned*, unsigned*,
                                      const FinHead*);
template void launch_atr_prox<float>(const GemmPlan&, const float*, const float*, float*,
                                     const float*, float*, float*, float*, double, double, double,
                                     Red, hipStream_t, Pub, float*, unsigned*, unsigned*, const FinHead*);

// the head kernel of the plan's tile: workgroups a CU holds at once, and the device's CUs
void atr_prox_head_capacity(const GemmPlan& p, int* cus, int* per_cu) {
  *cus = 0;
  *per_cu = 0;
  if (!atr_prox_head_ok(p, 1, 1)) return;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    *cus = 0;
    return;
  }
  atr_visit<double, true>(p, "fused A^T R + trial", [&](auto i, auto nt) {
    constexpr const AtrTile& tile = kAtrTiles[decltype(i)::value];
    if constexpr (tile.wl == 0)
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
              per_cu, k_atr_prox_head<decltype(nt)::value, tile.pf, tile.ntl>, 256, 0) != hipSuccess)
        *per_cu = 0;
  });
}
template void launch_atr<float>(const GemmPlan&, const float*, const float*, float*, hipStream_t);


}  // namespace glx

GLX_CLK_READER(glx_probe_clock_atr)
