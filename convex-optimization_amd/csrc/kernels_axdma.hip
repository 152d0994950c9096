// kernels_axdma.hip — A @ X (reference: gl_ProxGD_primal.py:25,61,129 `A @ x`) with A and X
// staged in LDS by LDS-DMA, f64 and f32 (the Dma family of glx_tiles.h, planned in planner.cpp).
#include "glx_mfma.h"

namespace glx {

// ------------------------------------------------------------------------------------------
// A @ X, kind 8 (f64): A and X staged in LDS by LDS-DMA (global_load_lds_dwordx4). The kind-5
// tile loads A straight into the MFMA operand registers, so one wave-instruction can only
// cover 16 rows x 64 B (a lane's bytes must be its own row's); the streaming probe
// (scripts/stream_probe.hip, profiles/r2_stream/) caps that shape at 5.9-6.2 TB/s against
// 6.3-7.3 TB/s for whole 256-512-B pieces. Here the wave-instruction that fetches A is decoupled
// from the lane that consumes it: each instruction lands 4 rows x 256 B (KC = 32) in LDS and
// the lanes read their MFMA operands back with ds_read_b128.
//
// Block = WAVES waves; wave w owns 16 rows (row0 .. row0 + 15) and streams them itself; the
// block's X chunk (KC rows of every source) is fetched by one 1-KiB instruction per wave and
// shared. A ring of NS LDS slots, NS - 1 chunks in flight. Per chunk every wave waits for its
// own DMAs of that chunk with a counted vmcnt, then ONE raw s_barrier (never __syncthreads(),
// whose fence waits for vmcnt(0) and would drain the ring) makes every wave's DMAs visible,
// then the next chunk is issued into the slot the previous chunk used (every wave has read it:
// its ds_reads completed before the wave reached the barrier, lgkmcnt(0) in the same wait).
//
// LDS images (one __shared__ array; the DMA destination is lane-linear, so swizzles go on the
// SOURCE address, cdna_hip_programming.md §5.4 rule 21):
//   A: wave's [16][SLR] 16-B slots (SLR = KC / EV, EV = 16 / sizeof(T) values per slot), slot s
//      of row i stored at s ^ sw(i). Lane (i, q) reads slots s = q + 4j (j < SLR / 4), i.e.
//      k = EV s + e — conflict-free ds_read_b128 for every 4 x 16-lane group
//      (MI355X_MICROARCH.md §LDS), checked by scripts/lds_banks.py. f32 with KC = 64 has the
//      same byte image as f64 with KC = 32 (256-B row pieces).
//   X: per source KC rows of l values as 16-value units of UB = 16 sizeof(T) bytes (k * NT +
//      half); unit u stored at u ^ ((k / EV) & (EV - 1)). f64 (ds_read_b64): the two 16-lane
//      halves of a group (lane groups q = 0/1 and 2/3 read rows k = 2(q + 4j) + e) fall on
//      different bank halves; f32 (ds_read_b32, all 64 lanes at once): the four lane groups'
//      64-B units (rows k = 4(q + 4j) + e) land on the four different 16-bank quarters.
// MFMA operand maps as in kind 5 (k permuted inside a chunk, X read with the same permutation).
// Past the end of a block's K range the ring re-issues the last chunk (an L2 hit, discarded),
// so every wave's DMA count per chunk is the same constant the counted vmcnt needs.
// ------------------------------------------------------------------------------------------
typedef __attribute__((address_space(1))) void g_void_t;
typedef __attribute__((address_space(3))) void l_void_t;

// one 16-B-per-lane LDS-DMA wave-instruction: lane j writes lds_base + 16 j (lds_base uniform)
template <bool NTL>
__device__ inline void glds16(const void* src, void* lds_base) {
  __builtin_amdgcn_global_load_lds((g_void_t*)src, (l_void_t*)lds_base, 16, 0, NTL ? 2 : 0);
}

// LDS bytes of a kind-8 tile: NS slots of WAVES 16-row A chunks + the X chunk of every source
// (+ 1 KiB dummy when the X pieces do not divide evenly among the waves)
template <typename T, int NT, int NSRC, int NS, int KC, int WAVES, int MT = 1>
constexpr int dma_lds_bytes() {
  constexpr int es = (int)sizeof(T);
  return NS * (WAVES * 16 * MT * KC * es + NSRC * KC * 16 * NT * es) +
         ((NSRC * KC * 16 * NT * es / 1024) % WAVES ? 1024 : 0);
}

// Infinity-Cache hand-off (GemmPlan::ax_keep_mib, a kernel argument; the solver's default is
// kKeepMiB = 192, GLX_AX_KEEP_MIB overrides it, 0 = off): with NTL, the last chunks of every
// block's walk are fetched with the default policy instead, about that many MiB of A over the
// grid, so they stay in the 256 MiB Infinity Cache for the next pass (A^T R).

// a wave-uniform pointer taken to SGPRs
__device__ inline const char* sgpr_ptr(const char* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return reinterpret_cast<const char*>(((uint64_t)hi << 32) | lo);
}

// A slot swizzle of row i for SLR 16-B slots per row piece
template <int SLR>
__device__ inline int dma_sw(int i) { return SLR >= 16 ? (i & 15) : ((i >> 1) & 7); }

template <typename T, int NT, int NSRC, int NS, int KC, int WAVES, bool NTL, bool HOIST, bool PIPE,
          int MT, bool EG = false>
__global__ __launch_bounds__(64 * WAVES) void k_ax_dma(const T* __restrict__ A,
                                                      const T* __restrict__ X0,
                                                      const T* __restrict__ X1,
                                                      const T* __restrict__ X2,
                                                      T* __restrict__ P, int64_t m, int64_t n,
                                                      int64_t chunks, int S, int gx, int xmap,
                                                      const int* __restrict__ gate, int epoch,
                                                      Pub pub, int keep_mib, EGat eg) {
  typedef MF<T> M;
  typedef typename M::acc_t C;
  typedef typename M::vec_t V;                      // one 16-B slot of A
  constexpr int ES = (int)sizeof(T);
  constexpr int EV = 16 / ES;                       // values per 16-B slot (2 f64, 4 f32)
  constexpr int UB = 16 * ES;                       // bytes of one 16-value X unit
  constexpr int LPU = UB / 16;                      // DMA lanes per X unit
  constexpr int UPI = 1024 / UB;                    // X units per DMA wave-instruction
  constexpr int L = 16 * NT;
  constexpr int NC = NT * NSRC;
  constexpr int SLR = KC / EV;                      // 16-B slots per row of an A chunk
  constexpr int AW = 16 * MT * KC * (int)sizeof(T); // one wave's A chunk (MT 16-row tiles)
  constexpr int NIA = AW / 1024;                    // its LDS-DMA instructions
  constexpr int XS = KC * L * (int)sizeof(T);       // one source's X chunk
  constexpr int XB = NSRC * XS;
  constexpr int NXT = XB / 1024;                    // the block's X instructions per chunk
  constexpr int NIX = (NXT + WAVES - 1) / WAVES;    // per wave (surplus ones load a dummy)
  constexpr bool XDUP = NIX * WAVES != NXT;
  constexpr int SLOT = WAVES * AW + XB;
  constexpr int LDSB = NS * SLOT + (XDUP ? 1024 : 0);
  constexpr int NI = NIA + NIX;                     // DMA instructions per wave and chunk
  constexpr int D = NS - 1;                         // chunks in flight beyond the computed one
  constexpr int JN = SLR / 4;                       // ds_read_b128 of A per lane and chunk
  constexpr int WAITN = (D - 1) * NI;
  static_assert(KC == 16 || KC == 32 || KC == 64, "chunk of 16, 32 or 64 columns");
  static_assert(XS % 1024 == 0 && AW % 1024 == 0, "whole 1-KiB pieces");
  static_assert(D >= 1 && WAITN <= 63, "vmcnt range");
  static_assert(LDSB <= 160 * 1024, "LDS");
  static_assert(MT == 1 || PIPE, "two row tiles per wave: pipelined form only");
  static_assert(!EG || (NSRC == 1 && PIPE && HOIST && NS == 2 && KC == 32 && 64 % L == 0),
                "the fused A e: one MFMA source, the pipelined two-slot tile");
  // PIPE && HOIST: the pipelined loop with the DMA issues and operand reads interleaved into
  // the MFMA stream (sched_group_barrier) instead of all issued in front of it
  // s_waitcnt vmcnt(WAITN) expcnt(7) lgkmcnt(0) (gfx9 encoding: vmcnt[3:0] bits 3:0, expcnt
  // bits 6:4, lgkmcnt bits 11:8, vmcnt[5:4] bits 15:14)
  constexpr int kWaitVmLgkm0 = (WAITN & 15) | (7 << 4) | ((WAITN >> 4) << 14);
  __shared__ __attribute__((aligned(1024))) char lds[LDSB];

  GLX_CLK(0);
  if (pub.host != nullptr && blockIdx.x == 0) {   // as k_ax_lds: workgroup 0 carries the packet
    if (threadIdx.x == 0)
      publish_packet(pub.s, pub.ns, pub.host, pub.host_seq, pub.seq, pub.s2, pub.off2, pub.n2,
                     pub.s3, pub.off3, pub.n3);
    return;
  }
  if (!gate_live(gate, epoch)) return;
  int bx, by;
  if (!ax_block(xmap, gx, S, bx, by, pub.host != nullptr ? 1 : 0)) return;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, q = lane >> 4;
  const int64_t row0 = (int64_t)bx * (16 * MT * WAVES) + (int64_t)wave * (16 * MT);
  const int64_t cb = chunks * by / S, ce = chunks * (by + 1) / S;
  const int64_t nch = ce - cb;
  if (nch <= 0) return;   // block-uniform

  // A piece t of this wave: linear slot 64 t + lane of the [16][SLR] image
  // Its source is a wave-uniform base (the wave's first row, the split's first chunk: SGPRs,
  // advanced per chunk by scalar adds) plus a loop-invariant 32-bit byte offset per lane (the
  // launcher checks that 16 MT rows fit one), the SGPR-base form of the global load: one VGPR per
  // piece and no 64-bit vector add per chunk.
  const int64_t rowb = row0 < m ? row0 : m - 1;
  const char* const abase = sgpr_ptr(reinterpret_cast<const char*>(A + rowb * n + cb * KC));
  unsigned aoffs[NIA];
#pragma unroll
  for (int t = 0; t < NIA; ++t) {
    const int ls = 64 * t + lane, ri = ls / SLR, p = ls % SLR;
    int64_t r = row0 + ri;
    r = r < m ? r : m - 1;
    aoffs[t] = (unsigned)(((r - rowb) * n + EV * (p ^ dma_sw<SLR>(ri & 15))) * ES);
  }
  // X pieces: instruction tx = wave + WAVES r of the block covers the UPI units UPI tx ..
  // (an instruction lies within one source, so its base is wave-uniform too: as for A)
  static_assert((KC * NT) % UPI == 0, "an X instruction within one source");
  const char* xbase[NIX];
  unsigned xoffs[NIX];
  int xdst[NIX];
#pragma unroll
  for (int r = 0; r < NIX; ++r) {
    const int tx = wave + WAVES * r;
    const int txc = tx % NXT;                        // surplus: a real piece into the dummy
    const int pu = UPI * txc + lane / LPU;
    const int src = (UPI * txc) / (KC * NT), u = pu % (KC * NT);
    const int k = u / NT;
    const int us = u ^ ((k / EV) & (EV - 1));
    const T* xb = src == 0 ? X0 : (src == 1 ? X1 : X2);
    xbase[r] = sgpr_ptr(reinterpret_cast<const char*>(xb + cb * KC * L));
    xoffs[r] = (unsigned)(((us / NT) * L + (us % NT) * 16 + (lane % LPU) * EV) * ES);
    xdst[r] = tx < NXT ? WAVES * AW + tx * 1024 : -1;
  }
  const int64_t rot = ax_rot(xmap, bx, gx, nch);
  int64_t kt = nch;   // walk chunks [kt, nch) load with the default policy (the hand-off)
  if constexpr (NTL) {
    const int64_t kb = (int64_t)keep_mib << 20;
    if (kb > 0) kt = nch - kb / ((int64_t)gridDim.x * WAVES * AW);
  }
  // walk step j loads A non-temporally while its (clamped) chunk lies below kt: block-uniform
  auto step_nt = [&](int64_t j) -> bool { return NTL && (j < nch ? j : nch - 1) < kt; };
  // the NI DMAs of walk step c into ring slot `slot`, A's policy a compile-time argument (one
  // basic block: the pipelined loop's sched_group_barrier sequence places every one of them)
  auto issue_as = [&](auto ntp, int64_t c, int slot) {
    constexpr bool NTP = decltype(ntp)::value;
    c = c < nch ? c : nch - 1;
    c += rot;                            // the walk starts at chunk rot (mod nch)
    c = c >= nch ? c - nch : c;
    c = __builtin_amdgcn_readfirstlane((int)c);   // a chunk index of the split: fits an int
    char* sb = lds + slot * SLOT;
    const char* const ab = abase + c * (KC * ES);
#pragma unroll
    for (int t = 0; t < NIA; ++t) {
      // (opaque here, so the zero extension stays next to the add and is matched as the load's
      // 32-bit offset operand instead of being hoisted into a loop-invariant 64-bit pair)
      unsigned off = aoffs[t];
      asm("" : "+v"(off));
      glds16<NTP>(ab + off, sb + wave * AW + t * 1024);
    }
#pragma unroll
    for (int r = 0; r < NIX; ++r) {
      unsigned off = xoffs[r];
      asm("" : "+v"(off));
      glds16<false>(xbase[r] + c * (KC * L * ES) + off, XDUP && xdst[r] < 0 ? lds + NS * SLOT : sb + xdst[r]);
    }
  };
  auto issue = [&](int64_t c, int slot) {   // the policy looked up at run time (prologue, flat loop)
    if (step_nt(c)) issue_as(std::bool_constant<NTL>{}, c, slot);
    else issue_as(std::false_type{}, c, slot);
  };

  C acc[MT][NC];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[mt][c] = C{};

  // lane (i, q): A slots q + 4j of row i; X units of rows k = EV (q + 4j) + e, whose swizzle
  // (k / EV) & (EV - 1) = q & (EV - 1)
  const int aoff = wave * AW + i * (SLR * 16);
  int asl[MT][JN];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < JN; ++j) asl[mt][j] = aoff + mt * 16 * SLR * 16 + 16 * ((q + 4 * j) ^ dma_sw<SLR>(i));
  const int xoff = WAVES * AW + ES * i;
  const int xq = q & (EV - 1);
  auto compute = [&](int slot) {
    const char* sb = lds + slot * SLOT;
    V av[JN];
#pragma unroll
    for (int j = 0; j < JN; ++j) av[j] = *reinterpret_cast<const V*>(sb + asl[0][j]);
    if constexpr (HOIST) {
      // every LDS read of the chunk first, in MFMA order, then the MFMAs: the compiler's counted
      // lgkmcnt waits then retire them progressively instead of a wait per small read group
      T xv[JN][EV][NSRC][NT];
#pragma unroll
      for (int j = 0; j < JN; ++j)
#pragma unroll
        for (int e = 0; e < EV; ++e)
#pragma unroll
          for (int src = 0; src < NSRC; ++src)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              const int k = EV * (q + 4 * j) + e;
              const int unit = (k * NT + nt) ^ xq;
              xv[j][e][src][nt] = *reinterpret_cast<const T*>(sb + xoff + src * XS + unit * UB);
            }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < JN; ++j)
#pragma unroll
        for (int e = 0; e < EV; ++e)
#pragma unroll
          for (int src = 0; src < NSRC; ++src)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              acc[0][src * NT + nt] = M::mma(av[j][e], xv[j][e][src][nt], acc[0][src * NT + nt]);
      return;
    }
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
      for (int e = 0; e < EV; ++e) {
        const int k = EV * (q + 4 * j) + e;
#pragma unroll
        for (int src = 0; src < NSRC; ++src)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const int unit = (k * NT + nt) ^ xq;
            const T xv = *reinterpret_cast<const T*>(sb + xoff + src * XS + unit * UB);
            acc[0][src * NT + nt] = M::mma(av[j][e], xv, acc[0][src * NT + nt]);
          }
      }
  };

  // ---- EG: the MFMA source X0 is the candidate p itself (A p: the objective and the Armijo test)
  // and A e, e = p where the hard threshold zeroes it, is accumulated on VALU from the staged
  // chunks, by the block as a whole: after the barrier every wave's A chunk image is visible to
  // every wave, and the images of the WAVES waves are contiguous ([16 MT WAVES][SLR] slots), so
  // wave v owns the CPW = L / WAVES COLUMNS v CPW .. v CPW + CPW - 1 of e for all the block's
  // rows, and lane i the RG = 16 MT WAVES / 64 rows i, i + 64, .. of them: accE[RG][CPW], every
  // index static. The bitmap is tested on the scalar side: lane c < L loads the u32 of column c's
  // bitmap that covers the chunk's 32 k (one chunk ahead, like the DMA ring, so the barrier's
  // wait covers it); at the chunk the wave takes the words of its own CPW columns to SGPRs with
  // readlane and skips the walk whole where they are all zero (with about one entry per flagged
  // row and eight flagged rows per chunk late in a solve, a wave meets about one entry per
  // chunk, where a wave that owned rows met all eight). Else its columns are visited in a
  // statically unrolled loop and the set bits k of a word in a wave-uniform loop, ascending. Per
  // entry (k, c) the wave issues one broadcast read of p[k][c] from the staged X chunk (source
  // 0 = p), RG ds_read_b64 of A[i + 64 g][k] (the lane's row base plus the uniform k under dma_sw,
  // the row groups 64 rows = an immediate offset apart: conflict-free over 16 rows, two-way over
  // 32) and accE[g][c - v CPW] += A[i + 64 g][k] p[k][c] in all 64 lanes. A chunk's walk runs
  // inside the MFMA stream of the chunk before it, the two waves of a SIMD at different points
  // (the pipelined loop below).
  // Order of summation of every (row, column) accumulator: (1) per K split, the block's (rotated)
  // chunk walk; (2) ascending k within a chunk; (3) one rounded multiply and one rounded add per
  // entry (-ffp-contract=off). The finalize sums the S slabs in order and forms
  // A p_thr - b = (A p - b) - A e.
  static_assert(!EG || ((16 * MT * WAVES) % 64 == 0 && L % WAVES == 0 && AW == 16 * MT * SLR * 16),
                "the fused A e: whole 64-row groups, whole columns per wave, contiguous images");
  constexpr int RG = EG ? (16 * MT * WAVES) / 64 : 1;
  constexpr int CPW = EG ? L / WAVES : 1;
  T accE[RG][CPW];
#pragma unroll
  for (int g = 0; g < RG; ++g)
#pragma unroll
    for (int j = 0; j < CPW; ++j) accE[g][j] = T(0);
  const int ecol_c = lane % L;
  const unsigned short* ecol = EG ? eg.bm + (int64_t)ecol_c * eg.bstride : nullptr;
  auto ebits = [&](int64_t c) -> unsigned {   // bitmap word of walk step c (0 past the range)
    if constexpr (!EG) {
      return 0u;
    } else {
      const bool in = c < nch;           // branch-free: the clamped word is loaded, 0 selected
      c = in ? c : nch - 1;
      c += rot;
      c = c >= nch ? c - nch : c;
      const unsigned w = *reinterpret_cast<const unsigned*>(ecol + (cb + c) * (KC / 16));
      return in ? w : 0u;
    }
  };
  auto ework = [&](int slot, unsigned bits) __attribute__((always_inline)) {
    if constexpr (EG) {
      unsigned wd[CPW], any = 0u;
#pragma unroll
      for (int j = 0; j < CPW; ++j) {
        wd[j] = (unsigned)__builtin_amdgcn_readlane((int)bits, wave * CPW + j);
        any |= wd[j];
      }
      if (any == 0u) return;   // wave-uniform, as every branch below
      const char* sb = lds + slot * SLOT;
      const char* arow = sb + lane * (SLR * 16);
      const int esw = dma_sw<SLR>(lane & 15);
#pragma unroll
      for (int j = 0; j < CPW; ++j) {
        const int c = wave * CPW + j;
        unsigned w = wd[j];
        while (w != 0u) {
          const int kk = __builtin_ctz(w);
          w &= w - 1u;
          const int unit = (kk * NT + (c >> 4)) ^ ((kk / EV) & (EV - 1));
          // e[k][c] = p[k][c] where the bitmap is set: one address for the whole wave
          const T ev = *reinterpret_cast<const T*>(sb + WAVES * AW + unit * UB + (c & 15) * ES);
          const int ao = 16 * ((kk / EV) ^ esw) + ES * (kk % EV);
          T ar[RG];
#pragma unroll
          for (int g = 0; g < RG; ++g) ar[g] = *reinterpret_cast<const T*>(arow + g * 64 * (SLR * 16) + ao);
#pragma unroll
          for (int g = 0; g < RG; ++g) accE[g][j] = accE[g][j] + ar[g] * ev;
        }
      }
    }
  };
  unsigned ebr[2] = {0u, 0u};   // bitmap words of the next two walk steps
  (void)ebr;

  if constexpr (PIPE) {
    // Software-pipelined: the operands of chunk c sit in registers (read one iteration earlier)
    // when chunk c's MFMAs issue, so the MFMA pipe does not idle on the LDS read latency after
    // each barrier (the two waves of a SIMD reach it in lockstep); chunk c + 1's reads are
    // issued in front of those MFMAs and complete behind them. Same ring: after the barrier of
    // iteration c every wave has landed chunk c + 1 and finished reading chunk c, whose slot
    // takes chunk c + 1 + D.
    // (fp64 MFMA on live data holds the clock near 2.05-2.2 GHz, where A@X's 2 m n l flops
    // need ~125 us of MFMA pipe against ~158 us of streaming: scripts/axdma_ablate.hip.)
    V av[2][MT][JN];
    T xv[2][JN][EV][NSRC][NT];
    auto read_ops = [&](int slot, V (&a)[MT][JN], T (&x)[JN][EV][NSRC][NT]) {
      const char* sb = lds + slot * SLOT;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < JN; ++j) a[mt][j] = *reinterpret_cast<const V*>(sb + asl[mt][j]);
#pragma unroll
      for (int j = 0; j < JN; ++j)
#pragma unroll
        for (int e = 0; e < EV; ++e)
#pragma unroll
          for (int src = 0; src < NSRC; ++src)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              const int k = EV * (q + 4 * j) + e;
              const int unit = (k * NT + nt) ^ xq;
              x[j][e][src][nt] = *reinterpret_cast<const T*>(sb + xoff + src * XS + unit * UB);
            }
    };
    auto mma_ops = [&](const V (&a)[MT][JN], const T (&x)[JN][EV][NSRC][NT]) {
#pragma unroll
      for (int j = 0; j < JN; ++j)
#pragma unroll
        for (int e = 0; e < EV; ++e)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int src = 0; src < NSRC; ++src)
#pragma unroll
              for (int nt = 0; nt < NT; ++nt)
                acc[mt][src * NT + nt] = M::mma(a[mt][j][e], x[j][e][src][nt], acc[mt][src * NT + nt]);
    };
    // the MFMAs [lo, hi) of a chunk, in mma_ops' order
    auto mma_range = [&](const V (&a)[MT][JN], const T (&x)[JN][EV][NSRC][NT], auto lo, auto hi) __attribute__((always_inline)) {
#pragma unroll
      for (int f = decltype(lo)::value; f < decltype(hi)::value; ++f) {
        const int nt = f % NT, src = f / NT % NSRC, mt = f / (NT * NSRC) % MT;
        const int e = f / (NT * NSRC * MT) % EV, j = f / (NT * NSRC * MT * EV);
        acc[mt][src * NT + nt] = M::mma(a[mt][j][e], x[j][e][src][nt], acc[mt][src * NT + nt]);
      }
    };
    const int epar = (wave >> 2) & 1;   // the two waves of a SIMD (w, w + 4) take the walk at different points
    GLX_CLK(1);
    if constexpr (EG) ebr[0] = ebits(0);
#pragma unroll
    for (int d = 0; d < D; ++d) issue(d, d);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAITN) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (EG) ebr[1] = ebits(1);
    issue(D, D);          // NS = D + 1: slot D is free
    read_ops(0, av[0], xv[0]);
    if constexpr (EG) ework(0, ebr[0]);   // chunk 0 before the loop's first barrier frees slot 0
    int cs = 1;           // slot of chunk c + 1
    int64_t c = 0;
    // One step of the walk: chunk c + h in register set h, the DMAs of walk step c + h + 1 + D
    // issued with A's load policy NTP. h and the policy are compile-time arguments, so the part
    // from the barrier to the last MFMA is one basic block and HOIST's sched_group_barrier
    // sequence reaches every DMA (a run-time policy test inside would split the block and leave
    // all the A pieces in front of the first MFMA).
    auto step = [&](auto hh, auto ntp, int64_t c) __attribute__((always_inline)) {
      constexpr int h = decltype(hh)::value;
      // chunk c + h + 1 landed everywhere, chunk c + h no longer read by anyone. The builtin
      // (not inline asm) so that the compiler's own wait insertion knows the operand reads of
      // the previous iteration are complete and adds no lgkmcnt(0) in front of the MFMAs
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(kWaitVmLgkm0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      const int is = cs == 0 ? NS - 1 : cs - 1;   // slot of chunk c + h = slot of c + h + 1 + D
      unsigned eb_use = 0u;
      if constexpr (EG) {   // this step's word (chunk c + h + 1) out, the word of c + h + 2 in
        eb_use = ebr[h ^ 1];
        ebr[h] = ebits(c + h + 1 + D);
      }
      issue_as(ntp, c + h + 1 + D, is);
      read_ops(cs, av[h ^ 1], xv[h ^ 1]);         // next chunk's operands ...
      if constexpr (!HOIST) {
        __builtin_amdgcn_sched_barrier(0);        // (DMA and reads issue before the MFMAs)
        mma_ops(av[h], xv[h]);                    // ... in flight behind this chunk's MFMAs
      } else if constexpr (EG) {
        // As below, and chunk c + h + 1's A e (slot cs) goes INTO the MFMA stream, at a different
        // point for each of the two waves of a SIMD (w and w + 4): while one walks its entries
        // (LDS latency chains, the wave issues no MFMA) the other still has MFMAs to issue and the
        // pipe stays busy. Behind the last MFMA both waves walked at once and the pipe idled for
        // it. The points lie in the last quarter of the stream: the walk's registers (RG + 1
        // values) then fit into operands of this chunk that are already dead (at l = 32: 256
        // VGPRs, no scratch; at NMF * 5 / 8 and * 13 / 16 the kernel spilled four).
        constexpr int NMF = MT * JN * EV * NSRC * NT;
        constexpr int NRD = MT * JN + JN * EV * NSRC * NT;
        constexpr int MA = NMF - NMF / 4, MB = NMF - NMF / 8;
        static_assert(0 < MA && MA < MB && MB < NMF, "MFMAs left behind both walks");
        const bool walk = c + h + 1 < nch;
        mma_range(av[h], xv[h], std::integral_constant<int, 0>{}, std::integral_constant<int, MA>{});
#pragma unroll
        for (int g = 0; g < NI; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // 1 VMEM read (the DMA)
        }
#pragma unroll
        for (int g = 0; g < (NRD + 1) / 2; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // 2 DS reads
        }
        __builtin_amdgcn_sched_barrier(0);
        if (walk && epar == 0) ework(cs, eb_use);
        __builtin_amdgcn_sched_barrier(0);
        mma_range(av[h], xv[h], std::integral_constant<int, MA>{}, std::integral_constant<int, MB>{});
        __builtin_amdgcn_sched_barrier(0);
        if (walk && epar != 0) ework(cs, eb_use);
        __builtin_amdgcn_sched_barrier(0);
        mma_range(av[h], xv[h], std::integral_constant<int, MB>{}, std::integral_constant<int, NMF>{});
      } else {
        // An LDS-DMA issue costs its wave ~60-185 cycles (MI355X_MICROARCH.md constants):
        // spread the NI DMAs over the first MFMAs (one after each), then the operand reads two
        // per MFMA, so the issue costs hide under the MFMA pipe instead of delaying it
        mma_ops(av[h], xv[h]);
        constexpr int NMF = MT * JN * EV * NSRC * NT;      // MFMAs per chunk and wave
        constexpr int NRD = MT * JN + JN * EV * NSRC * NT; // operand reads per chunk and wave
#pragma unroll
        for (int g = 0; g < NI; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // 1 VMEM read (the DMA)
        }
#pragma unroll
        for (int g = 0; g < (NRD + 1) / 2; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // 2 DS reads
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NMF - NI - (NRD + 1) / 2, 0);
      }
      cs = cs + 1 == NS ? 0 : cs + 1;
    };
    // two chunks per trip so the register sets keep static indices
    auto trip = [&](auto nt0, auto nt1, int64_t c) __attribute__((always_inline)) {
      step(std::integral_constant<int, 0>{}, nt0, c);
      step(std::integral_constant<int, 1>{}, nt1, c);
    };
    // The walk split by load policy (the hand-off above): trips whose two issues (walk steps
    // c + 1 + D, c + 2 + D) are both non-temporal, at most one mixed trip, then trips that issue
    // with the default policy. step_nt is monotone in the step, and c, nch, kt are block-uniform,
    // so every wave of the block takes the same trips and meets the same barriers.
    // The trip counts are formed once, on the scalar side: of the ntr = nch / 2 trips, trip i
    // (c = 2 i) is all non-temporal while step_nt(2 i + 2 + D), i.e. for all of them where
    // kt >= nch and else for the i with 2 i + 2 + D < kt, floor((kt - 1 - D) / 2) of them.
    const int ntr = __builtin_amdgcn_readfirstlane((int)(nch >> 1));
    int n1 = 0, nmix = 0;
    if constexpr (NTL) {
      const int64_t below = (kt - 1 - D) >> 1;
      n1 = kt >= nch ? ntr : (int)(below < 0 ? 0 : (below < ntr ? below : ntr));
      n1 = __builtin_amdgcn_readfirstlane(n1);
      nmix = __builtin_amdgcn_readfirstlane(n1 < ntr && step_nt(2 * (int64_t)n1 + 1 + D) ? 1 : 0);
    }
    for (int i = 0; i < n1; ++i, c += 2) trip(std::true_type{}, std::true_type{}, c);
    if (nmix != 0) {
      trip(std::true_type{}, std::false_type{}, c);
      c += 2;
    }
    for (int i = n1 + nmix; i < ntr; ++i, c += 2) trip(std::false_type{}, std::false_type{}, c);
    if (c < nch) mma_ops(av[0], xv[0]);   // odd count: the last chunk is in set 0
    GLX_CLK(2);
  } else {
#pragma unroll
  for (int d = 0; d < D; ++d) issue(d, d);
  int cs = 0;
  for (int64_t c = 0; c < nch; ++c) {
    // this wave's DMAs of chunk c have landed (the D - 1 younger chunks may be in flight) and
    // its reads of chunk c - 1 are done; the barrier publishes both block-wide
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(WAITN) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int is = cs == 0 ? NS - 1 : cs - 1;   // slot of chunk c - 1 = slot of chunk c + D
    issue(c + D, is);
    compute(cs);
    cs = cs + 1 == NS ? 0 : cs + 1;
  }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the surplus re-issues, before exit
  if constexpr (EG) {   // wave v, lane i: its CPW contiguous columns of the block's rows i + 64 g
    T* pe = static_cast<T*>(eg.Pe) + (int64_t)by * m * L;
#pragma unroll
    for (int g = 0; g < RG; ++g) {
      const int64_t row = (int64_t)bx * (16 * MT * WAVES) + g * 64 + lane;
      if (row < m) {
#pragma unroll
        for (int j = 0; j < CPW; ++j) pe[row * L + wave * CPW + j] = accE[g][j];
      }
    }
  }

#pragma unroll
  for (int sr = 0; sr < NSRC; ++sr) {
    T* pout = P + ((int64_t)sr * S + by) * m * L;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + mt * 16 + M::row(lane, r);
        if (row < m) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) pout[row * L + nt * 16 + i] = acc[mt][sr * NT + nt][r];
        }
      }
  }
  GLX_CLK(3);
}

// The launcher takes its tile as the index I into kAxTiles (glx_tiles.h) and reads the kernel's
// template arguments and the grid geometry from that record.
template <typename T, int NT, int NSRC, std::size_t I, bool EG = false>
static void ax_dma_go(const GemmPlan& p, int S, const T* A, const T* const* X, T* P,
                      const int* gate, int epoch, hipStream_t st, Pub pub, const EGat& eg = EGat{}) {
  constexpr const AxTile& t = kAxTiles[I];
  if constexpr (dma_lds_bytes<T, NT, NSRC, t.slots, t.kc, t.waves, t.mt>() > 160 * 1024) {
    throw Error{GLX_E_INVALID, "A@X: this LDS-DMA tile does not fit (160 KiB of LDS)"};
  } else {
    // a lane's source offset from its wave's base (up to 16 MT rows of A) is a 32-bit value
    if ((uint64_t)p.n * (16 * t.mt) * sizeof(T) >= (1ull << 32))
      throw Error{GLX_E_INVALID, "A@X: rows of A too long for the LDS-DMA tile's 32-bit lane offsets"};
    const int gx = (int)cdiv(p.m, ax_tile_rows(t));
    const int xmap = ax_xmap_flags(p, S);
    const dim3 grid((unsigned)ax_grid(xmap, gx, S) + (pub.host ? 1u : 0u));
    glx_launch((k_ax_dma<T, NT, NSRC, t.slots, t.kc, t.waves, t.ntl, t.hoist, t.pipe, t.mt, EG>), grid,
               dim3(64 * t.waves), 0, st, A, X[0], X[1], X[2], P, p.m, p.n, p.n / t.kc, S, gx, xmap, gate, epoch,
               pub, p.ax_keep_mib, eg);
  }
}

template <typename T>
bool launch_ax_dma(const GemmPlan& p, const AxTile* tile, int nsrc, int S, const T* A, const T* const* X,
                   T* P, const int* gate, int epoch, hipStream_t st, Pub pub) {
  bool built = false;
  visit_tile(kAxTiles, tile, [&](auto i) {
    constexpr const AxTile& t = kAxTiles[decltype(i)::value];
    if constexpr (t.fam == Fam::Dma && (t.built & dtype_bit(sizeof(T))) != 0) {
      with_const<1, 2>((int)(p.l / 16), [&](auto nt) {
        with_const<1, 2, 3>(nsrc, [&](auto ns) {
          if constexpr (decltype(ns)::value <= t.nsrc_max) {
            ax_dma_go<T, decltype(nt)::value, decltype(ns)::value, decltype(i)::value>(p, S, A, X, P, gate, epoch,
                                                                                    st, pub);
            built = true;
          }
        });
      });
    }
  });
  return built;
}

// the fused A e form of the one-source f64 pass 92278 (EGat; ax_egat_ok: that is the plan's tile)
template <typename T>
bool launch_ax_egat(const GemmPlan& p, const T* A, const T* X, T* P, const int* gate, int epoch,
                    hipStream_t st, Pub pub, const EGat& eg) {
  if constexpr (sizeof(T) != 8) {
    return false;
  } else {
    if (!ax_egat_ok(p, 8)) return false;
    const T* xs[3] = {X, nullptr, nullptr};
    constexpr std::size_t kDma = ax_tile(92278) - kAxTiles;
    with_const<1, 2>((int)(p.l / 16), [&](auto nt) {
      ax_dma_go<T, decltype(nt)::value, 1, kDma, true>(p, p.axb_S[1], A, xs, P, gate, epoch, st, pub, eg);
    });
    return true;
  }
}
template bool launch_ax_egat<double>(const GemmPlan&, const double*, const double*, double*, const int*, int,
                                     hipStream_t, Pub, const EGat&);
template bool launch_ax_egat<float>(const GemmPlan&, const float*, const float*, float*, const int*, int,
                                    hipStream_t, Pub, const EGat&);

template bool launch_ax_dma<double>(const GemmPlan&, const AxTile*, int, int, const double*, const double* const*,
                                    double*, const int*, int, hipStream_t, Pub);
template bool launch_ax_dma<float>(const GemmPlan&, const AxTile*, int, int, const float*, const float* const*,
                                   float*, const int*, int, hipStream_t, Pub);

}  // namespace glx

GLX_CLK_READER(glx_probe_clock_ax)
