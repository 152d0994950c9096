// glx_tiles.h — the tiles of the two dense products, each defined once (host side only). A
// tile's numeric code is a label that is looked up here, never taken apart ("Tiles and
// the planner"); planner and launchers read a tile's parameters from its record.
#pragma once

#include <cstddef>
#include <type_traits>
#include <utility>

namespace glx {

enum class Fam { Valu, Mfma, Lds, Dma };   // VALU / direct-load MFMA / X in LDS / A and X by LDS-DMA
enum : unsigned { kF32 = 1u, kF64 = 2u, kAnyType = 3u };
constexpr unsigned dtype_bit(int esize) { return esize == 8 ? kF64 : kF32; }

// ---- A @ X ----
struct AxTile {
  int code;
  Fam fam;
  int mt;       // 16-row tiles per wave
  int pf;       // register ring depth in chunks (Mfma, Lds)
  int vpl;      // 16-B vectors a lane streams from its row per chunk (Mfma, Lds)
  int waves;    // per workgroup (Mfma: the 4 waves split the block's K chunks)
  int slots;    // Dma: LDS ring slots (NS)
  int kc;       // Dma: columns of A per chunk
  bool ntl;     // non-temporal A loads
  bool hoist, pipe;   // Dma: hoisted / pipelined operand reads
  unsigned dtypes;    // dtypes the planner admits the tile for
  unsigned built;     // dtypes its kernels are compiled for
  int nsrc_min, nsrc_max;   // right-hand sides per pass
  // Dma: the HOIST value describe_plan has always printed (1 for 92278 / 92268, 3 for 92478,
  // though all three are hoisted and pipelined): recorded plan strings key profiles/
  int shown_hoist;
};
inline constexpr AxTile kAxTiles[] = {
  // code  family     MT PF VPL  W  NS  KC   ntl   hoist  pipe   planner   built     nsrc  shown
  {3,     Fam::Valu, 0, 0, 0,  4, 0,  0,  false, false, false, kAnyType, kAnyType, 1, 3, 0},
  // direct loads into the MFMA operand registers: only where no LDS tile fits the shape (n not
  // a multiple of the LDS chunk); 1420 / 1220 are the batched forms (2 / 3 right-hand sides)
  {1820,  Fam::Mfma, 8, 2, 1,  4, 0,  0,  false, false, false, kAnyType, kAnyType, 1, 1, 0},
  {21820, Fam::Mfma, 8, 2, 2,  4, 0,  0,  false, false, false, kAnyType, kAnyType, 1, 1, 0},
  {21410, Fam::Mfma, 4, 1, 2,  4, 0,  0,  false, false, false, kAnyType, kAnyType, 1, 1, 0},
  {1420,  Fam::Mfma, 4, 2, 1,  4, 0,  0,  false, false, false, kAnyType, kAnyType, 2, 2, 0},
  {1220,  Fam::Mfma, 2, 2, 1,  4, 0,  0,  false, false, false, kAnyType, kAnyType, 3, 3, 0},
  // X staged in LDS: 52228 (f64 batched / one RHS in the Infinity Cache), 52224 (its 4-wave
  // form for deep-split shards), 51328 (one 16-row tile per wave: the one-RHS and shard tile at
  // l = 32), 52324 (f32 batched)
  {52228, Fam::Lds,  2, 2, 2,  8, 0,  0,  false, false, false, kAnyType, kAnyType, 1, 3, 0},
  {51328, Fam::Lds,  1, 3, 2,  8, 0,  0,  false, false, false, kAnyType, kAnyType, 1, 3, 0},
  {52324, Fam::Lds,  2, 3, 2,  4, 0,  0,  false, false, false, kAnyType, kAnyType, 1, 3, 0},
  {52224, Fam::Lds,  2, 2, 2,  4, 0,  0,  false, false, false, kAnyType, kAnyType, 1, 3, 0},
  // LDS-DMA, two row tiles per wave, 256-B row pieces, DMA issues interleaved into the MFMAs:
  // 92278 non-temporal A, 92268 the default load policy, 92478 f32 (round 4: 64-column chunks,
  // the same byte image as 92278 in f64; one source). The round-3 sweep's other forms (one row
  // tile per wave, 3-4 ring slots, 16-wave blocks, 16-column chunks, no hoisting / pipelining)
  // measured slower and are no longer built. The f64 tiles are still compiled for
  // f32, where the planner never admits them.
  {92278, Fam::Dma,  2, 0, 0,  8, 2,  32, true,  true,  true,  kF64,     kAnyType, 1, 3, 1},
  {92268, Fam::Dma,  2, 0, 0,  8, 2,  32, false, true,  true,  kF64,     kAnyType, 1, 3, 1},
  {92478, Fam::Dma,  2, 0, 0,  8, 2,  64, true,  true,  true,  kF32,     kF32,     1, 1, 3},
};
constexpr int ax_tile_rows(const AxTile& t) { return 16 * t.mt * (t.fam == Fam::Mfma ? 1 : t.waves); }
// k values per chunk of the tile's walk
constexpr int ax_tile_chunk(const AxTile& t, int esize) {
  return t.fam == Fam::Dma ? t.kc : 4 * (16 / esize) * t.vpl;
}

// ---- A^T R ----
struct AtrTile {
  int code;          // the GLX_ATR_VARIANT label
  Fam fam;           // Valu or Mfma
  int wl;            // wave layout: 0 four waves split a panel's rows, 1 four panels per block share
                     // rows, 2 eight waves per panel, 3 the 32-column panel (four waves)
  int pf;            // in-place ring depth (lookahead PF - 1 row steps)
  bool ntl;          // non-temporal A loads
  int panel;         // columns per panel
  int cols;          // columns per workgroup: n must be a multiple
  unsigned dtypes;   // dtypes k_atr_mfma is built (and planned) for
  unsigned fused;    // dtypes the fused-trial kernels (k_atr_prox, k_atr_fista) are built for
  int fallback;      // the tile planned instead where the dtype or n does not admit this one
};
// Round 6: only the tiles the planner picks are built — the f64
// default (WL 0, PF 8; non-temporal A beyond the Infinity Cache), the f32 default (WL 1, PF 4,
// non-temporal), the fp32 fused trial's eight-wave panel (WL 2) and the f64 32-column panel
// (WL 3). The measured-slower ring depths (PF 2-6) and the 8-wave 32-column panel (WL 4) of
// rounds 1-5 are gone; their numbers stay in DESIGN.md's tuning record.
inline constexpr AtrTile kAtrTiles[] = {
  // code family     WL PF ntl    panel cols built     fused     fallback
  {3,    Fam::Valu, 0, 0, false, 0,   1,   kAnyType, 0u,       3},
  {8,    Fam::Mfma, 0, 8, false, 64,  64,  kAnyType, kF64,     8},
  {1008, Fam::Mfma, 0, 8, true,  64,  64,  kAnyType, kAnyType, 1008},
  {1114, Fam::Mfma, 1, 4, true,  64,  256, kAnyType, 0u,       1008},
  {1028, Fam::Mfma, 2, 8, true,  64,  64,  kAnyType, kAnyType, 1028},
  {38,   Fam::Mfma, 3, 8, false, 32,  32,  kF64,     kF64,     8},
  {1038, Fam::Mfma, 3, 8, true,  32,  32,  kF64,     kF64,     1008},
};
// Labels of pruned tiles that recorded runs carry (profiles/), each with the built
// tile that has run under it since the pruning. Any other label plans kAtrUnknown.
constexpr int kAtrOldLabels[][2] = {{108, 8},    {104, 8},     {106, 8},    {24, 1028},
                                    {28, 1028},  {1024, 1028}, {114, 1114}, {1048, 1008}};
constexpr int kAtrUnknown = 1008;

// ---- lookup (plan time only; constexpr, so a launcher can name a tile by its code) ----
constexpr const AxTile* ax_tile(int code) {
  for (const AxTile& t : kAxTiles)
    if (t.code == code) return &t;
  return nullptr;
}
constexpr const AtrTile* atr_tile(int code) {
  for (const auto& old : kAtrOldLabels)
    if (old[0] == code) code = old[1];
  for (const AtrTile& t : kAtrTiles)
    if (t.code == code) return &t;
  return nullptr;
}

// f(std::integral_constant<size_t, I>) for the I with &tab[I] == t: the callee reads the record
// as a compile-time constant (kernel<..., tab[I].mt, tab[I].pf>); false: t is not in tab
template <typename Tile, std::size_t N, typename F, std::size_t... I>
inline bool visit_tile_seq(const Tile (&tab)[N], const Tile* t, F&& f, std::index_sequence<I...>) {
  return ((t == &tab[I] && (f(std::integral_constant<std::size_t, I>{}), true)) || ...);
}
template <typename Tile, std::size_t N, typename F>
inline bool visit_tile(const Tile (&tab)[N], const Tile* t, F&& f) {
  return visit_tile_seq(tab, t, std::forward<F>(f), std::make_index_sequence<N>{});
}

}  // namespace glx
