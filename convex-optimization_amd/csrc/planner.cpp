// planner.cpp — the launch planner of the two dense products (host only): which tile of
// glx_tiles.h runs A @ X and A^T R for a (dtype, m, n, l), with how many splits, and what it carries.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "glx_internal.h"

namespace glx {
namespace {

// Read once per planning call and never cached: tests change the environment between calls in
// one process. (GLX_FUSED_TRIAL is the session's knob; its presence is an override here.)
struct Knobs {
  EnvInt ax_variant{"GLX_AX_VARIANT"}, axb_variant{"GLX_AXB_VARIANT"}, atr_variant{"GLX_ATR_VARIANT"},
      ax_s{"GLX_AX_S"}, axb_s{"GLX_AXB_S"}, atr_s{"GLX_ATR_S"}, axl_blocks{"GLX_AXL_BLOCKS"},
      ax_dma{"GLX_AX_DMA"}, ax_dma32{"GLX_AX_DMA32"}, shard_tile{"GLX_SHARD_TILE"}, ax_xcd{"GLX_AX_XCD"},
      ax_rot{"GLX_AX_ROT"}, atr_narrow{"GLX_ATR_NARROW"}, atr_fuse_split{"GLX_ATR_FUSE_SPLIT"},
      fused_trial{"GLX_FUSED_TRIAL"};
};

// ---- defaults (sweep in scripts/kbench.py on MI355X) ----
// The f64 LDS default falls back to the dtype's direct-load tile when the shape does not fit it
// (n not a multiple of the tile's chunk; l not 16/32 is VALU).
constexpr const AxTile* kAxDefault = ax_tile(52228);
const AxTile* ax_direct(int esize) { return ax_tile(esize == 8 ? 21820 : 21410); }
constexpr int kAtrDefault = 108;        // f64: WL 0, PF 8 (A that stays in the MALL)
constexpr int kAtrDefaultBig = 1008;    // f64: non-temporal A, WL 0, PF 8
// Non-temporal A loads pay only when A cannot stay in the 256 MiB Infinity Cache between the
// passes: NS (1 GiB) 2278 -> 2326 it/s, FProxGD 2397 -> 2451, but C2 (256 MiB) 7477 -> 6250 and
// the 1024-row shard (128 MiB) 9477 -> 8323 (profiles/r2_axat/)
constexpr double kAtrNtBytes = 384.0 * 1024 * 1024;
constexpr int kAtrDefault32 = 1114;     // f32: non-temporal A, WL 1, PF 4
// batched right-hand sides (MFMA-bound at l = 32, both dtypes): the LDS tile, 2 waves per SIMD
// (end-to-end sweep, profiles/r1_tuning: f64 8-wave blocks, f32 4-wave blocks with PF 3)
const AxTile* axb_default(int esize) { return esize == 8 ? kAxDefault : ax_tile(52324); }
// the 4-wave LDS tile of a dtype (deep-split shards, lds_plan)
const AxTile* ax_lds4(int esize) { return esize == 8 ? ax_tile(52224) : ax_tile(52324); }

bool mfma_l(int64_t l) { return l == 16 || l == 32; }
bool lds_fam(const AxTile* t) { return t != nullptr && (t->fam == Fam::Lds || t->fam == Fam::Dma); }

// LDS bytes of an LDS-DMA tile for l columns and nsrc right-hand sides (kernels_axdma.hip
// dma_lds_bytes): ring slots of every wave's A chunk + every source's X chunk (+ 1 KiB dummy)
int dma_lds_need(const AxTile& t, int64_t l, int nsrc, int esize) {
  const int xb = nsrc * t.kc * (int)l * esize;
  return t.slots * (t.waves * 16 * t.mt * t.kc * esize + xb) + ((xb / 1024) % t.waves ? 1024 : 0);
}
// an LDS / LDS-DMA tile takes this shape
bool lds_tile_ok(const AxTile* t, int64_t n, int64_t l, int esize, int nsrc = 1) {
  if (!lds_fam(t) || !mfma_l(l) || n % ax_tile_chunk(*t, esize) != 0) return false;
  if (t->fam == Fam::Lds) return true;
  return (t->dtypes & dtype_bit(esize)) != 0 && nsrc <= t->nsrc_max &&
         dma_lds_need(*t, l, nsrc, esize) <= 160 * 1024;
}
// K split of an LDS / LDS-DMA launch: enough blocks for 2 (4-wave) blocks per CU
int lds_split(const Knobs& k, int esize, int64_t m, int64_t n, const AxTile& t, int64_t target = 0) {
  const int64_t rb = cdiv(m, ax_tile_rows(t)), chunks = n / ax_tile_chunk(t, esize);
  if (target <= 0) target = k.axl_blocks.or_(t.waves >= 8 ? 256 : 512);
  return (int)clampi(cdiv(target, rb), 1, std::max<int64_t>(1, std::min<int64_t>(kMaxSplit, chunks / 8)));
}
// A K-split launch writes S partial slabs of m x (nsrc*l) that the finalize kernel reads back.
// With few rows (the per-rank shards of a multi-GPU run) a 256-block target lets S reach 64 and
// the slabs rival A itself. When they exceed 1/6 of A, use the 4-wave tile at 256 blocks, which
// halves them. Shard-shape sweep (profiles/r1_tuning/shard_shapes.txt): at m = 1024 this is
// +10 % end to end despite a slower A@X; at m >= 2048 the default tile stays ahead.
//
// Per-rank shards at l = 32 (m <= 2048: the 4- and 8-GPU runs of the north-star size) take the
// 8-wave tile with ONE 16-row tile per wave and a 3-deep ring (51328): at these row counts the
// K splits are short, and two waves per SIMD with half the rows per block keep the slab volume
// of the 4-wave tile. Measured end to end with the communicator path
// (profiles/r1_tuning/small_kernels/ax_shard_tile.log): +4.7 % at m = 1024, +3 % at 2048,
// neutral at 4096; at m = 8192 the default tile stays ahead (A@X 290 vs 306 us).
//
// One right-hand side at l = 32, f64 (round 2: the split-candidate trial's dense pass A p_thr is
// HBM-bound): 51328 with its 4 K splits, A@X 246-250 vs 252-254 us incl. the A e gather, NS
// ProxGD 2266-2269 vs 2231-2232 it/s on one box (profiles/r2_axtile/).
//
// Round 3, the LDS-DMA tile (kernels_axdma.hip): one right-hand side in fp64 with A beyond the
// Infinity Cache (the split-candidate dense pass A p_thr at NS, FProxGD's A xc, C5's shard) takes
// 92278 (two 16-row tiles per wave, 256-B row pieces, 2-slot ring, non-temporal A, DMA issues and
// operand reads interleaved into the MFMA stream): NS 164 vs 193-196 us (6.57 TB/s), the 16384-row
// shard 334 vs 399 us. fp64 C2 (two right-hand sides, l = 16, A in the Infinity Cache) takes
// 92268 (default policy): 46.2 vs 49.3 us. Interleaved kernel-trace A/B, profiles/r3_axdma/.
void lds_plan(const Knobs& k, int esize, int64_t m, int64_t n, int64_t l, int nsrc, const AxTile*& t,
              int& S) {
  S = lds_split(k, esize, m, n, *t);
  if (k.axl_blocks.set() || k.axb_variant.set()) return;
  auto take = [&](const AxTile* c) { t = c; S = lds_split(k, esize, m, n, *c); };
  const bool big = (double)m * (double)n * esize > kAtrNtBytes;
  const bool f64_default = esize == 8 && t == kAxDefault;
  if (f64_default && nsrc == 1 && big && lds_tile_ok(ax_tile(92278), n, l, esize, 1) && k.ax_dma.on() &&
      !k.ax_variant.set())
    return take(ax_tile(92278));
  if (f64_default && nsrc == 2 && l == 16 && !big && lds_tile_ok(ax_tile(92268), n, l, esize, 2) && k.ax_dma.on())
    return take(ax_tile(92268));
  if (f64_default && nsrc == 1 && l == 32 && lds_tile_ok(ax_tile(51328), n, l, esize) && !k.ax_variant.set())
    return take(ax_tile(51328));
  if (f64_default && nsrc == 2 && l == 32 && m <= 2048 && lds_tile_ok(ax_tile(51328), n, l, esize) && k.shard_tile.on())
    return take(ax_tile(51328));
  if ((double)S * (double)m * nsrc * l * 6.0 <= (double)m * n) return;
  const AxTile* c4 = ax_lds4(esize);
  if (!lds_tile_ok(c4, n, l, esize)) return;
  const int S4 = lds_split(k, esize, m, n, *c4, 256);
  if (S4 < S) { t = c4; S = S4; }
}

// VALU column block width (1, 2, 4, 8) for l columns
int valu_lb(int64_t l) {
  if (l == 3) return 4;
  return l > 4 ? 8 : (l >= 4 ? 4 : (l >= 2 ? 2 : 1));
}

GemmPlan plan(const Knobs& k, int esize, int64_t m, int64_t n, int64_t l, int ax_variant) {
  GemmPlan p{};
  p.esize = esize;
  p.m = m; p.n = n; p.l = l;
  const int E = 16 / esize;
  const bool big = (double)m * (double)n * esize > kAtrNtBytes;
  // ---- A @ X ----
  // the request: a tile's code; 0 = the planner's choice; 1, 2 = the dtype's direct-load tile
  const int req = ax_variant != 0 ? ax_variant : k.ax_variant.or_(0);
  const AxTile *direct = ax_direct(esize), *valu = ax_tile(3), *dma32 = ax_tile(92478);
  const AxTile* want = (req == 1 || req == 2) ? direct : ax_tile(req);   // null: 0, or no such tile
  const bool valu_req = want != nullptr && want->fam == Fam::Valu;
  const bool ax_mfma_ok = mfma_l(l) && (n % (4 * E) == 0);
  const AxTile* lds = req != 0 ? want : (esize == 8 ? kAxDefault : direct);
  if (valu_req || !ax_mfma_ok) {
    p.ax[1] = valu;
    p.ax_lb = valu_lb(l);
    p.ax_vec = (n % E == 0) ? 1 : 0;
    const int64_t waves = cdiv(m, 4);                    // RW = 4 rows per wave
    const int64_t kunits = n / (64 * (p.ax_vec ? E : 1)); // 64-lane strides per row
    p.ax_S = (int)clampi(cdiv(kTargetWaves, waves), 1, std::max<int64_t>(1, std::min<int64_t>(kMaxSplit, kunits / 4)));
  } else if (esize == 4 && req == 0 && big && lds_tile_ok(dma32, n, l, esize, 1) && k.ax_dma.on() &&
             k.ax_dma32.on()) {
    // Round 4: f32 with one right-hand side and A beyond the Infinity Cache (C3's split-candidate
    // dense pass A xc) on the LDS-DMA tile, as 92278 does for f64: 85-88 us = 6.1-6.3 TB/s
    // against 115 us for the direct-load tile 21410 (profiles/r4_exp3/). GLX_AX_DMA32=0: off.
    p.ax[1] = dma32;
    p.ax_S = lds_split(k, esize, m, n, *dma32);
  } else if (lds_tile_ok(lds, n, l, esize)) {
    p.ax[1] = lds;
    if (req != 0) p.ax_S = lds_split(k, esize, m, n, *lds);
    else lds_plan(k, esize, m, n, l, 1, p.ax[1], p.ax_S);
  } else {
    // direct-load tiles: the one asked for if it is a one-source tile, else the dtype's
    const AxTile* t = (want != nullptr && want->fam == Fam::Mfma && want->nsrc_min == 1) ? want : direct;
    if (n % ax_tile_chunk(*t, esize) != 0) t = ax_tile(1820);   // wider chunks need n % 4*E*VPL
    p.ax[1] = t;
    const int64_t blocks = cdiv(m, ax_tile_rows(*t));
    const int64_t chunks = n / ax_tile_chunk(*t, esize);
    // sweep (scripts/kbench.py): f64 at MT 8 wants 1024 waves, f32 4096
    const int64_t target = esize == 8 ? (t->mt == 8 ? kTargetWaves / 2 : kTargetWaves) : 2 * kTargetWaves;
    p.ax_S = (int)clampi(cdiv(target, blocks * 4), 1,
                         std::max<int64_t>(1, std::min<int64_t>(kMaxSplit, chunks / 16)));
  }
  if (k.ax_s.or_(0) > 0) p.ax_S = (int)std::min<int64_t>(k.ax_s.or_(0), kMaxSplit);
  p.ax_xmap = (k.ax_xcd.on() ? 1 : 0) | (k.ax_rot.on() ? 2 : 0);
  // batched right-hand sides. A direct-load label here only names the plan: launch_ax has one
  // direct-load batch kernel per source count (1420 / 1220) and runs that.
  p.axb_S[0] = p.axb_S[1] = p.ax_S;
  for (int ns = 2; ns <= 3; ++ns) {
    const AxTile* t = k.axb_variant.or_(0) != 0 ? ax_tile(k.axb_variant.or_(0)) : axb_default(esize);
    const AxTile* fallback = ax_tile(ns == 2 ? 1420 : 1220);
    int S = p.ax_S;
    if (p.ax[1]->fam == Fam::Valu) {
      t = valu;
    } else if (lds_fam(t)) {
      if (lds_tile_ok(t, n, l, esize, ns)) lds_plan(k, esize, m, n, l, ns, t, S);
      else t = fallback;
    } else if (t == nullptr || t->fam != Fam::Mfma || n % ax_tile_chunk(*t, esize) != 0) {
      t = fallback;
    }
    if (k.axb_s.or_(0) > 0 && lds_fam(t)) S = (int)std::min<int64_t>(k.axb_s.or_(0), kMaxSplit);
    p.ax[ns] = t;
    p.axb_S[ns] = S;
  }
  // ---- A^T R ----
  int label = k.atr_variant.or_(0);
  if (label == 0) label = esize == 8 ? (big ? kAtrDefaultBig : kAtrDefault) : kAtrDefault32;
  const AtrTile* t = atr_tile(label);
  if (t == nullptr) t = atr_tile(kAtrUnknown);
  // four shared-row panels need n % 256, the 32-column panel is f64: else the tile's fallback
  if ((t->dtypes & dtype_bit(esize)) == 0 || n % t->cols != 0) t = atr_tile(t->fallback);
  const bool atr_mfma_ok = mfma_l(l) && (n % 64 == 0) && (m % 4 == 0);
  if (valu_req || t->fam == Fam::Valu || !atr_mfma_ok) {
    p.atr = atr_tile(3);
    p.atr_lb = valu_lb(l);
    p.atr_vec = (n % E == 0) ? 1 : 0;
    const int64_t cols_per_block = 256 * (p.atr_vec ? E : 1);
    const int64_t blocks = cdiv(n, cols_per_block);
    p.atr_S = (int)clampi(cdiv(kTargetWaves / 4, blocks), 1, std::max<int64_t>(1, std::min<int64_t>(kMaxSplit, m / 16)));
  } else {
    p.atr = t;
    const int64_t steps = m / 4, blocks = n / t->cols;
    // f64: one wave per SIMD is enough with the PF-8 ring (and S = 1 at n = 16384 lets the
    // ProxGD trial fuse into the kernel); f32 wants 4 per SIMD. Four panels per block (WL 1):
    // a quarter of the blocks
    const int64_t target = esize == 8 ? kTargetWaves / 2 : 2 * kTargetWaves;
    const int64_t want_S = t->wl == 1 ? cdiv(kTargetWaves / 4, blocks) : cdiv(target, blocks * 4);
    p.atr_S = (int)clampi(want_S, 1, std::max<int64_t>(1, std::min<int64_t>(kMaxSplit, steps / 16)));
  }
  if (k.atr_s.or_(0) > 0) p.atr_S = (int)std::min<int64_t>(k.atr_s.or_(0), kMaxSplit);
  return p;
}

std::string ax_name(const GemmPlan& p, int nsrc) {
  const AxTile& t = *p.ax[nsrc];
  const int S = ax_split(p, nsrc);
  char buf[128];
  switch (t.fam) {
    case Fam::Valu:
      std::snprintf(buf, sizeof buf, "k_ax_valu<LB%d,VEC%d> S=%d", p.ax_lb, p.ax_vec, S);
      break;
    case Fam::Dma:
      std::snprintf(buf, sizeof buf, "k_ax_dma<MT%d,NS%d,KC%d,NTL%d,HOIST%d(2:PIPE),W%d> S=%d", t.mt, t.slots,
                    t.kc, (int)t.ntl, t.shown_hoist, t.waves, S);
      break;
    case Fam::Lds:
      std::snprintf(buf, sizeof buf, "k_ax_lds<MT%d,PF%d,VPL%d,W%d> S=%d", t.mt, t.pf, t.vpl, t.waves, S);
      break;
    case Fam::Mfma:   // kind 1: direct row loads (the quad-load kind 2 is no longer built)
      std::snprintf(buf, sizeof buf, "k_ax_mfma<kind1,MT%d,PF%d,NTL%d,VPL%d> S=%d", t.mt, t.pf, (int)t.ntl,
                    t.vpl, S);
      break;
  }
  return buf;
}

// a trial fuses into this plan's A^T R: MFMA panels that are not shared-row (WL 1), at most 8 K
// splits with a slab combine (GLX_ATR_FUSE_SPLIT=0: none), none on the 32-column f64 panel
bool fuses(const EnvInt& fuse_split, const GemmPlan& p) {
  const AtrTile& t = *p.atr;
  if (t.fam != Fam::Mfma || t.wl == 1 || (t.wl == 3 && p.esize != 8)) return false;
  const int max_S = t.wl == 3 ? 1 : 8;
  return p.atr_S >= 1 && p.atr_S <= max_S && mfma_l(p.l) && p.n % t.panel == 0 &&
         p.n / t.panel < kMaxBlocks &&   // reducing slots (one per panel) + the publisher
         (p.atr_S == 1 || fuse_split.on());
}

}  // namespace

GemmPlan make_plan(int esize, int64_t m, int64_t n, int64_t l, int v) { return plan(Knobs{}, esize, m, n, l, v); }

// The method-level A^T R choice of a session: where ProxGD's / FProxGD's trial can fuse into
// A^T R (one GPU, no override present), take the tile and split measured best for the fused pass.
GemmPlan session_plan(const glx_problem& P, const glx_opts& O) {
  const Knobs k{};
  const int es = P.dtype == GLX_F64 ? 8 : 4;
  const GemmPlan p = plan(k, es, P.m, P.n, P.l, O.ax_variant);
  const bool trial_method = (P.method == GLX_PROXGD || P.method == GLX_FPROXGD) &&
                            (O.step_type == GLX_STEP_LINE_SEARCH || O.step_type == GLX_STEP_FIXED);
  if (P.comm != nullptr || !trial_method || p.atr->fam != Fam::Mfma || !mfma_l(P.l) || k.atr_variant.set() ||
      k.atr_s.set() || k.fused_trial.set())
    return p;
  auto with = [&](int label, int S) { GemmPlan f = p; f.atr = atr_tile(label); f.atr_S = S; return f; };
  if (es == 4 && P.n % 64 == 0 && P.m >= 128 && (P.n / 64) * 2 < kMaxBlocks) {
    // fp32: WL 0 with non-temporal A, the PF 8 ring (round 3) and two K splits (1008, S = 2).
    // Round 4: with at least one panel per CU, the eight-wave panel (WL 2: two waves per SIMD)
    // with one K split, no slab combine (1028, S = 1): C3 FProxGD A^T R + trial 101.2-101.4 us
    // against 107.4-107.6, 3815-3825 against 3741-3748 it/s over 200 steps (profiles/r4_c3atr/;
    // with two K splits it measured 119 us, with the PF 4 ring 104 us)
    // (round 6: a sixteen-step ring, twice the A bytes in flight per wave, measured slower:
    // A^T R + trial 120.9 against 101.3 us at C3, 3 628 against 3 862 it/s, profiles/r6_egat/)
    const GemmPlan f = P.n / 64 >= 256 ? with(1028, 1) : with(1008, 2);
    if (fuses(k.atr_fuse_split, f)) return f;   // only where the trial actually fuses (GLX_ATR_FUSE_SPLIT)
  }
  // Round 5: fp64 with fewer than 256 64-column panels (C2: 128, planned as 2 K splits) takes
  // the 32-column panel without K splits (WL 3; 38 / 1038: the planned tile's load policy): 256+
  // workgroups and no slab combine in front of the fused trial. GLX_ATR_NARROW=0: off. (Its
  // eight-wave form, WL 4, measured slower and is no longer built, round 6.)
  if (es == 8 && P.n % 32 == 0 && P.n / 64 < 256 && P.n / 32 >= 256 && !(k.atr_narrow.set() && std::strcmp(k.atr_narrow.s, "0") == 0)) {
    const GemmPlan f = with(p.atr->ntl ? 1038 : 38, 1);
    if (fuses(k.atr_fuse_split, f)) return f;
  }
  return p;
}

std::string describe_plan(const GemmPlan& p) {
  std::string s;
  for (int ns = 1; ns <= 3; ++ns) s += "ax" + std::to_string(ns) + "=" + ax_name(p, ns) + "; ";
  const AtrTile& t = *p.atr;
  char buf[128];
  if (t.fam == Fam::Valu)
    std::snprintf(buf, sizeof buf, "atr=k_atr_valu<LB%d,VEC%d> S=%d", p.atr_lb, p.atr_vec, p.atr_S);
  else
    std::snprintf(buf, sizeof buf, "atr=k_atr_mfma<WL%d,PF%d,NTL%d> S=%d%s", t.wl, t.pf, (int)t.ntl, p.atr_S,
                  t.panel == 32 ? " (32-column panels)" : "");
  return s + buf;
}

int max_ax_split(int esize, int64_t m, int64_t n, int64_t l) {
  const Knobs k{};
  int s = ax_split_max(plan(k, esize, m, n, l, 0));
  for (const AxTile& t : kAxTiles) s = std::max(s, ax_split_max(plan(k, esize, m, n, l, t.code)));
  return s;
}

bool ax_pub_ok(const GemmPlan& p, int nsrc) { return mfma_l(p.l) && nsrc >= 1 && nsrc <= 3 && lds_fam(p.ax[nsrc]); }
bool ax_egat_ok(const GemmPlan& p, int esize) {
  return esize == 8 && p.ax[1] == ax_tile(92278) && mfma_l(p.l) && p.n % 32 == 0 && p.n <= 65535;
}
bool ax_derive_ok(const GemmPlan& p, int esize) { return esize == 8 && p.ax[1] == ax_tile(51328) && p.l == 32 && p.n % 16 == 0; }
bool atr_prox_ok(const GemmPlan& p) { return fuses(EnvInt{"GLX_ATR_FUSE_SPLIT"}, p); }
// the finalize head of the fused trial (kernels_atr.hip): built for the f64 four-wave 64-column
// panel without K splits, one lane per residual element (at most kSlabLoads = 8 slabs a source)
bool atr_prox_head_ok(const GemmPlan& p, int S, int S0) {
  return atr_prox_ok(p) && p.esize == 8 && p.atr->wl == 0 && p.atr_S == 1 && S >= 1 && S <= 8 && S0 >= 0 && S0 <= 8;
}
int atr_prox_slots(const GemmPlan& p, bool pub) {
  return (int)(p.n / (p.atr->panel ? p.atr->panel : 64)) + (pub ? 1 : 0);
}

}  // namespace glx
