"""The case table of the dense-product tile tests (test_tiles_cpu.py, test_gpu_tiles.py).

One row per admitted (product, tile code of csrc/glx_tiles.h, dtype, right-hand sides):
    (product, code, dtype, nsrc, plan, shapes)
``plan`` is what glx_plan_describe must show for that product ("ax<nsrc>=" or "atr=" in front),
with {S} the K split; ``shapes`` are (m, n, l, S) or (m, n, l, S, "KNOB=value ...") with the
environment the case sets. The VALU rows' kernel name depends on the shape (column block, vector
loads), so there plan is "{S}" and a shape's S is the whole string.

The shapes are derived from the tile's record, not from the workload. With RB = ax_tile_rows,
C = ax_tile_chunk and D the register ring depth pf (LDS-DMA: the LDS slots):
  A @ X, MFMA tiles   (1, C, 16) one row, one chunk; (6, (D - 1) C, 32) fewer chunks than the ring, a
                      row count below 16 that is no multiple of 4; (17, 3 C, 16) an odd count (three
                      chunks on the two-slot DMA ring); (17, C, 32); (RB + 1, 5 C, 32) a second row
                      block of one row, whole ring trips and a tail; (RB + 1, 25 C, 16) with S = 3
                      forced: 8 S + 1 chunks, which S does not divide. The direct-load tiles, whose
                      four waves split a block's chunks, also (17, 13 C, 16): three or four chunks per
                      wave, so the ring refills. The direct-load defaults (1820 / 1420 / 1220) only
                      run where n is no multiple of the LDS chunk: all their n are such.
  A @ X, VALU         l in {1, 3, 17} and l = 16 with ragged n, both VEC0 and VEC1, S = 3 forced.
  A^T R, MFMA tiles   row steps (m / 4) of 1, 3, 9, 37 (one K split forced: every wave walks more
                      than one ring of 8) and 25 with S = 3 forced; n in {64, 128, 256, 320}
                      (four shared-row panels: 256 only).
  A^T R, VALU         m that is no multiple of 4 at an MFMA-eligible (n, l); ragged n; S = 3 forced.
No forced split leaves a split without a chunk or a row step. The rest are the shapes whose plans
the planner picks on its own (S = 9 over 72 and 73 chunks, the DMA tile's S = 4).

The f64 LDS-DMA tiles 92278 / 92268 are compiled for f32 as well (AxTile::built), but no request
reaches them there: lds_tile_ok refuses a tile whose AxTile::dtypes lacks the dtype, for
GLX_AX_VARIANT and GLX_AXB_VARIANT alike. Admitted therefore means built and planned.
"""
import collections

KNOBS = ("GLX_AX_VARIANT", "GLX_AXB_VARIANT", "GLX_ATR_VARIANT", "GLX_AX_S", "GLX_AXB_S", "GLX_ATR_S")

ROWS = [
    ("ax", 3, "f64", 1, "{S}", [
        (1, 7, 1, "k_ax_valu<LB1,VEC0> S=1"), (6, 132, 3, "k_ax_valu<LB4,VEC1> S=1"),
        (17, 301, 17, "k_ax_valu<LB8,VEC0> S=1"), (5, 30, 16, "k_ax_valu<LB8,VEC1> S=1"),
        (18, 1000, 17, "k_ax_valu<LB8,VEC1> S=3", "GLX_AX_S=3")]),
    ("ax", 3, "f64", 2, "{S}", [
        (1, 7, 1, "k_ax_valu<LB1,VEC0> S=1"), (6, 132, 3, "k_ax_valu<LB4,VEC1> S=1"),
        (17, 301, 17, "k_ax_valu<LB8,VEC0> S=1"), (5, 30, 16, "k_ax_valu<LB8,VEC1> S=1"),
        (18, 1000, 17, "k_ax_valu<LB8,VEC1> S=3", "GLX_AX_S=3")]),
    ("ax", 3, "f64", 3, "{S}", [
        (1, 7, 1, "k_ax_valu<LB1,VEC0> S=1"), (6, 132, 3, "k_ax_valu<LB4,VEC1> S=1"),
        (17, 301, 17, "k_ax_valu<LB8,VEC0> S=1"), (5, 30, 16, "k_ax_valu<LB8,VEC1> S=1"),
        (18, 1000, 17, "k_ax_valu<LB8,VEC1> S=3", "GLX_AX_S=3")]),
    ("ax", 3, "f32", 1, "{S}", [
        (1, 7, 1, "k_ax_valu<LB1,VEC0> S=1"), (6, 132, 3, "k_ax_valu<LB4,VEC1> S=1"),
        (17, 301, 17, "k_ax_valu<LB8,VEC0> S=1"), (5, 30, 16, "k_ax_valu<LB8,VEC0> S=1"),
        (18, 1000, 17, "k_ax_valu<LB8,VEC1> S=3", "GLX_AX_S=3")]),
    ("ax", 3, "f32", 2, "{S}", [
        (1, 7, 1, "k_ax_valu<LB1,VEC0> S=1"), (6, 132, 3, "k_ax_valu<LB4,VEC1> S=1"),
        (17, 301, 17, "k_ax_valu<LB8,VEC0> S=1"), (5, 30, 16, "k_ax_valu<LB8,VEC0> S=1"),
        (18, 1000, 17, "k_ax_valu<LB8,VEC1> S=3", "GLX_AX_S=3")]),
    ("ax", 3, "f32", 3, "{S}", [
        (1, 7, 1, "k_ax_valu<LB1,VEC0> S=1"), (6, 132, 3, "k_ax_valu<LB4,VEC1> S=1"),
        (17, 301, 17, "k_ax_valu<LB8,VEC0> S=1"), (5, 30, 16, "k_ax_valu<LB8,VEC0> S=1"),
        (18, 1000, 17, "k_ax_valu<LB8,VEC1> S=3", "GLX_AX_S=3")]),
    ("ax", 1820, "f64", 1, "k_ax_mfma<kind1,MT8,PF2,NTL0,VPL1> S={S}", [
        (1, 8, 16, 1), (6, 8, 32, 1), (17, 24, 16, 1), (17, 8, 32, 1), (129, 40, 32, 1),
        (129, 200, 16, 3, "GLX_AX_S=3"), (17, 72, 16, 1), (17, 104, 16, 1)]),
    ("ax", 1820, "f32", 1, "k_ax_mfma<kind1,MT8,PF2,NTL0,VPL1> S={S}", [
        (1, 16, 16, 1), (6, 16, 32, 1), (17, 48, 16, 1), (17, 16, 32, 1), (129, 80, 32, 1),
        (129, 400, 16, 3, "GLX_AX_S=3"), (17, 208, 16, 1)]),
    ("ax", 21820, "f64", 1, "k_ax_mfma<kind1,MT8,PF2,NTL0,VPL2> S={S}", [
        (1, 16, 16, 1, "GLX_AX_VARIANT=21820"), (6, 16, 32, 1, "GLX_AX_VARIANT=21820"),
        (17, 48, 16, 1, "GLX_AX_VARIANT=21820"), (17, 16, 32, 1, "GLX_AX_VARIANT=21820"),
        (129, 80, 32, 1, "GLX_AX_VARIANT=21820"), (129, 400, 16, 3, "GLX_AX_VARIANT=21820 GLX_AX_S=3"),
        (17, 208, 16, 1, "GLX_AX_VARIANT=21820")]),
    ("ax", 21820, "f32", 1, "k_ax_mfma<kind1,MT8,PF2,NTL0,VPL2> S={S}", [
        (1, 32, 16, 1, "GLX_AX_VARIANT=21820"), (6, 32, 32, 1, "GLX_AX_VARIANT=21820"),
        (17, 96, 16, 1, "GLX_AX_VARIANT=21820"), (17, 32, 32, 1, "GLX_AX_VARIANT=21820"),
        (129, 160, 32, 1, "GLX_AX_VARIANT=21820"), (129, 800, 16, 3, "GLX_AX_VARIANT=21820 GLX_AX_S=3"),
        (17, 416, 16, 1, "GLX_AX_VARIANT=21820")]),
    ("ax", 21410, "f64", 1, "k_ax_mfma<kind1,MT4,PF1,NTL0,VPL2> S={S}", [
        (1, 16, 16, 1, "GLX_AX_VARIANT=21410"), (6, 16, 32, 1, "GLX_AX_VARIANT=21410"),
        (17, 48, 16, 1, "GLX_AX_VARIANT=21410"), (17, 16, 32, 1, "GLX_AX_VARIANT=21410"),
        (65, 80, 32, 1, "GLX_AX_VARIANT=21410"), (65, 400, 16, 3, "GLX_AX_VARIANT=21410 GLX_AX_S=3"),
        (17, 208, 16, 1, "GLX_AX_VARIANT=21410")]),
    ("ax", 21410, "f32", 1, "k_ax_mfma<kind1,MT4,PF1,NTL0,VPL2> S={S}", [
        (1, 32, 16, 1), (6, 32, 32, 1), (17, 96, 16, 1), (17, 32, 32, 1), (65, 160, 32, 1),
        (65, 800, 16, 3, "GLX_AX_S=3"), (17, 96, 32, 1), (17, 416, 16, 1)]),
    ("ax", 1420, "f64", 2, "k_ax_mfma<kind1,MT4,PF2,NTL0,VPL1> S={S}", [
        (1, 8, 16, 1), (6, 8, 32, 1), (17, 24, 16, 1), (17, 8, 32, 1), (65, 40, 32, 1),
        (65, 200, 16, 3, "GLX_AX_S=3"), (17, 72, 16, 1), (17, 104, 16, 1)]),
    ("ax", 1420, "f32", 2, "k_ax_mfma<kind1,MT4,PF2,NTL0,VPL1> S={S}", [
        (1, 16, 16, 1), (6, 16, 32, 1), (17, 48, 16, 1), (17, 16, 32, 1), (65, 80, 32, 1),
        (65, 400, 16, 3, "GLX_AX_S=3"), (17, 208, 16, 1)]),
    ("ax", 1220, "f64", 3, "k_ax_mfma<kind1,MT2,PF2,NTL0,VPL1> S={S}", [
        (1, 8, 16, 1), (6, 8, 32, 1), (17, 24, 16, 1), (17, 8, 32, 1), (33, 40, 32, 1),
        (33, 200, 16, 3, "GLX_AX_S=3"), (17, 72, 16, 1), (17, 104, 16, 1)]),
    ("ax", 1220, "f32", 3, "k_ax_mfma<kind1,MT2,PF2,NTL0,VPL1> S={S}", [
        (1, 16, 16, 1), (6, 16, 32, 1), (17, 48, 16, 1), (17, 16, 32, 1), (33, 80, 32, 1),
        (33, 400, 16, 3, "GLX_AX_S=3"), (17, 208, 16, 1)]),
    ("ax", 52228, "f64", 1, "k_ax_lds<MT2,PF2,VPL2,W8> S={S}", [
        (1, 16, 16, 1), (6, 16, 32, 1, "GLX_AX_VARIANT=52228"), (17, 48, 16, 1),
        (17, 16, 32, 1, "GLX_AX_VARIANT=52228"), (257, 80, 32, 1, "GLX_AX_VARIANT=52228"),
        (257, 400, 16, 3, "GLX_AX_S=3"), (33, 96, 16, 1), (33, 1152, 16, 9), (33, 384, 16, 3, "GLX_AX_S=3")]),
    ("ax", 52228, "f64", 2, "k_ax_lds<MT2,PF2,VPL2,W8> S={S}", [
        (1, 16, 16, 1), (6, 16, 32, 1, "GLX_AXB_VARIANT=52228"), (17, 48, 16, 1),
        (17, 16, 32, 1, "GLX_AXB_VARIANT=52228"), (257, 80, 32, 1, "GLX_AXB_VARIANT=52228"),
        (257, 400, 16, 3, "GLX_AXB_S=3")]),
    ("ax", 52228, "f64", 3, "k_ax_lds<MT2,PF2,VPL2,W8> S={S}", [
        (1, 16, 16, 1), (6, 16, 32, 1), (17, 48, 16, 1), (17, 16, 32, 1), (257, 80, 32, 1),
        (257, 400, 16, 3, "GLX_AXB_S=3"), (33, 32, 32, 1), (33, 96, 16, 1), (33, 1152, 16, 9), (200, 1168, 32, 9)]),
    ("ax", 52228, "f32", 1, "k_ax_lds<MT2,PF2,VPL2,W8> S={S}", [
        (1, 32, 16, 1, "GLX_AX_VARIANT=52228"), (6, 32, 32, 1, "GLX_AX_VARIANT=52228"),
        (17, 96, 16, 1, "GLX_AX_VARIANT=52228"), (17, 32, 32, 1, "GLX_AX_VARIANT=52228"),
        (257, 160, 32, 1, "GLX_AX_VARIANT=52228"), (257, 800, 16, 3, "GLX_AX_VARIANT=52228 GLX_AX_S=3")]),
    ("ax", 52228, "f32", 2, "k_ax_lds<MT2,PF2,VPL2,W8> S={S}", [
        (1, 32, 16, 1, "GLX_AXB_VARIANT=52228"), (6, 32, 32, 1, "GLX_AXB_VARIANT=52228"),
        (17, 96, 16, 1, "GLX_AXB_VARIANT=52228"), (17, 32, 32, 1, "GLX_AXB_VARIANT=52228"),
        (257, 160, 32, 1, "GLX_AXB_VARIANT=52228"), (257, 800, 16, 3, "GLX_AXB_VARIANT=52228 GLX_AXB_S=3")]),
    ("ax", 52228, "f32", 3, "k_ax_lds<MT2,PF2,VPL2,W8> S={S}", [
        (1, 32, 16, 1, "GLX_AXB_VARIANT=52228"), (6, 32, 32, 1, "GLX_AXB_VARIANT=52228"),
        (17, 96, 16, 1, "GLX_AXB_VARIANT=52228"), (17, 32, 32, 1, "GLX_AXB_VARIANT=52228"),
        (257, 160, 32, 1, "GLX_AXB_VARIANT=52228"), (257, 800, 16, 3, "GLX_AXB_VARIANT=52228 GLX_AXB_S=3")]),
    ("ax", 51328, "f64", 1, "k_ax_lds<MT1,PF3,VPL2,W8> S={S}", [
        (1, 16, 16, 1, "GLX_AX_VARIANT=51328"), (6, 32, 32, 1), (17, 48, 16, 1, "GLX_AX_VARIANT=51328"),
        (17, 16, 32, 1), (129, 80, 32, 1), (129, 400, 16, 3, "GLX_AX_VARIANT=51328 GLX_AX_S=3"), (33, 32, 32, 1),
        (200, 1168, 32, 9)]),
    ("ax", 51328, "f64", 2, "k_ax_lds<MT1,PF3,VPL2,W8> S={S}", [
        (1, 16, 16, 1, "GLX_AXB_VARIANT=51328"), (6, 32, 32, 1), (17, 48, 16, 1, "GLX_AXB_VARIANT=51328"),
        (17, 16, 32, 1), (129, 80, 32, 1), (129, 400, 16, 3, "GLX_AXB_VARIANT=51328 GLX_AXB_S=3"), (33, 32, 32, 1),
        (200, 1168, 32, 9)]),
    ("ax", 51328, "f64", 3, "k_ax_lds<MT1,PF3,VPL2,W8> S={S}", [
        (1, 16, 16, 1, "GLX_AXB_VARIANT=51328"), (6, 32, 32, 1, "GLX_AXB_VARIANT=51328"),
        (17, 48, 16, 1, "GLX_AXB_VARIANT=51328"), (17, 16, 32, 1, "GLX_AXB_VARIANT=51328"),
        (129, 80, 32, 1, "GLX_AXB_VARIANT=51328"), (129, 400, 16, 3, "GLX_AXB_VARIANT=51328 GLX_AXB_S=3")]),
    ("ax", 51328, "f32", 1, "k_ax_lds<MT1,PF3,VPL2,W8> S={S}", [
        (1, 32, 16, 1, "GLX_AX_VARIANT=51328"), (6, 64, 32, 1, "GLX_AX_VARIANT=51328"),
        (17, 96, 16, 1, "GLX_AX_VARIANT=51328"), (17, 32, 32, 1, "GLX_AX_VARIANT=51328"),
        (129, 160, 32, 1, "GLX_AX_VARIANT=51328"), (129, 800, 16, 3, "GLX_AX_VARIANT=51328 GLX_AX_S=3")]),
    ("ax", 51328, "f32", 2, "k_ax_lds<MT1,PF3,VPL2,W8> S={S}", [
        (1, 32, 16, 1, "GLX_AXB_VARIANT=51328"), (6, 64, 32, 1, "GLX_AXB_VARIANT=51328"),
        (17, 96, 16, 1, "GLX_AXB_VARIANT=51328"), (17, 32, 32, 1, "GLX_AXB_VARIANT=51328"),
        (129, 160, 32, 1, "GLX_AXB_VARIANT=51328"), (129, 800, 16, 3, "GLX_AXB_VARIANT=51328 GLX_AXB_S=3")]),
    ("ax", 51328, "f32", 3, "k_ax_lds<MT1,PF3,VPL2,W8> S={S}", [
        (1, 32, 16, 1, "GLX_AXB_VARIANT=51328"), (6, 64, 32, 1, "GLX_AXB_VARIANT=51328"),
        (17, 96, 16, 1, "GLX_AXB_VARIANT=51328"), (17, 32, 32, 1, "GLX_AXB_VARIANT=51328"),
        (129, 160, 32, 1, "GLX_AXB_VARIANT=51328"), (129, 800, 16, 3, "GLX_AXB_VARIANT=51328 GLX_AXB_S=3")]),
    ("ax", 52324, "f64", 1, "k_ax_lds<MT2,PF3,VPL2,W4> S={S}", [
        (1, 16, 16, 1, "GLX_AX_VARIANT=52324"), (6, 32, 32, 1, "GLX_AX_VARIANT=52324"),
        (17, 48, 16, 1, "GLX_AX_VARIANT=52324"), (17, 16, 32, 1, "GLX_AX_VARIANT=52324"),
        (129, 80, 32, 1, "GLX_AX_VARIANT=52324"), (129, 400, 16, 3, "GLX_AX_VARIANT=52324 GLX_AX_S=3")]),
    ("ax", 52324, "f64", 2, "k_ax_lds<MT2,PF3,VPL2,W4> S={S}", [
        (1, 16, 16, 1, "GLX_AXB_VARIANT=52324"), (6, 32, 32, 1, "GLX_AXB_VARIANT=52324"),
        (17, 48, 16, 1, "GLX_AXB_VARIANT=52324"), (17, 16, 32, 1, "GLX_AXB_VARIANT=52324"),
        (129, 80, 32, 1, "GLX_AXB_VARIANT=52324"), (129, 400, 16, 3, "GLX_AXB_VARIANT=52324 GLX_AXB_S=3")]),
    ("ax", 52324, "f64", 3, "k_ax_lds<MT2,PF3,VPL2,W4> S={S}", [
        (1, 16, 16, 1, "GLX_AXB_VARIANT=52324"), (6, 32, 32, 1, "GLX_AXB_VARIANT=52324"),
        (17, 48, 16, 1, "GLX_AXB_VARIANT=52324"), (17, 16, 32, 1, "GLX_AXB_VARIANT=52324"),
        (129, 80, 32, 1, "GLX_AXB_VARIANT=52324"), (129, 400, 16, 3, "GLX_AXB_VARIANT=52324 GLX_AXB_S=3")]),
    ("ax", 52324, "f32", 1, "k_ax_lds<MT2,PF3,VPL2,W4> S={S}", [
        (1, 32, 16, 1, "GLX_AX_VARIANT=52324"), (6, 64, 32, 1, "GLX_AX_VARIANT=52324"),
        (17, 96, 16, 1, "GLX_AX_VARIANT=52324"), (17, 32, 32, 1, "GLX_AX_VARIANT=52324"),
        (129, 160, 32, 1, "GLX_AX_VARIANT=52324"), (129, 800, 16, 3, "GLX_AX_VARIANT=52324 GLX_AX_S=3")]),
    ("ax", 52324, "f32", 2, "k_ax_lds<MT2,PF3,VPL2,W4> S={S}", [
        (1, 32, 16, 1), (6, 64, 32, 1), (17, 96, 16, 1), (17, 32, 32, 1), (129, 160, 32, 1),
        (129, 800, 16, 3, "GLX_AXB_S=3"), (17, 96, 32, 1)]),
    ("ax", 52324, "f32", 3, "k_ax_lds<MT2,PF3,VPL2,W4> S={S}", [
        (1, 32, 16, 1), (6, 64, 32, 1), (17, 96, 16, 1), (17, 32, 32, 1), (129, 160, 32, 1),
        (129, 800, 16, 3, "GLX_AXB_S=3"), (17, 96, 32, 1)]),
    ("ax", 52224, "f64", 1, "k_ax_lds<MT2,PF2,VPL2,W4> S={S}", [
        (1, 16, 16, 1, "GLX_AX_VARIANT=52224"), (6, 16, 32, 1, "GLX_AX_VARIANT=52224"),
        (17, 48, 16, 1, "GLX_AX_VARIANT=52224"), (17, 16, 32, 1, "GLX_AX_VARIANT=52224"),
        (129, 80, 32, 1, "GLX_AX_VARIANT=52224"), (129, 400, 16, 3, "GLX_AX_VARIANT=52224 GLX_AX_S=3")]),
    ("ax", 52224, "f64", 2, "k_ax_lds<MT2,PF2,VPL2,W4> S={S}", [
        (1, 16, 16, 1, "GLX_AXB_VARIANT=52224"), (6, 16, 32, 1, "GLX_AXB_VARIANT=52224"),
        (17, 48, 16, 1, "GLX_AXB_VARIANT=52224"), (17, 16, 32, 1, "GLX_AXB_VARIANT=52224"),
        (129, 80, 32, 1, "GLX_AXB_VARIANT=52224"), (129, 400, 16, 3, "GLX_AXB_VARIANT=52224 GLX_AXB_S=3")]),
    ("ax", 52224, "f64", 3, "k_ax_lds<MT2,PF2,VPL2,W4> S={S}", [
        (1, 16, 16, 1, "GLX_AXB_VARIANT=52224"), (6, 16, 32, 1, "GLX_AXB_VARIANT=52224"),
        (17, 48, 16, 1, "GLX_AXB_VARIANT=52224"), (17, 16, 32, 1, "GLX_AXB_VARIANT=52224"),
        (129, 80, 32, 1, "GLX_AXB_VARIANT=52224"), (129, 400, 16, 3, "GLX_AXB_VARIANT=52224 GLX_AXB_S=3")]),
    ("ax", 52224, "f32", 1, "k_ax_lds<MT2,PF2,VPL2,W4> S={S}", [
        (1, 32, 16, 1, "GLX_AX_VARIANT=52224"), (6, 32, 32, 1, "GLX_AX_VARIANT=52224"),
        (17, 96, 16, 1, "GLX_AX_VARIANT=52224"), (17, 32, 32, 1, "GLX_AX_VARIANT=52224"),
        (129, 160, 32, 1, "GLX_AX_VARIANT=52224"), (129, 800, 16, 3, "GLX_AX_VARIANT=52224 GLX_AX_S=3")]),
    ("ax", 52224, "f32", 2, "k_ax_lds<MT2,PF2,VPL2,W4> S={S}", [
        (1, 32, 16, 1, "GLX_AXB_VARIANT=52224"), (6, 32, 32, 1, "GLX_AXB_VARIANT=52224"),
        (17, 96, 16, 1, "GLX_AXB_VARIANT=52224"), (17, 32, 32, 1, "GLX_AXB_VARIANT=52224"),
        (129, 160, 32, 1, "GLX_AXB_VARIANT=52224"), (129, 800, 16, 3, "GLX_AXB_VARIANT=52224 GLX_AXB_S=3")]),
    ("ax", 52224, "f32", 3, "k_ax_lds<MT2,PF2,VPL2,W4> S={S}", [
        (1, 32, 16, 1, "GLX_AXB_VARIANT=52224"), (6, 32, 32, 1, "GLX_AXB_VARIANT=52224"),
        (17, 96, 16, 1, "GLX_AXB_VARIANT=52224"), (17, 32, 32, 1, "GLX_AXB_VARIANT=52224"),
        (129, 160, 32, 1, "GLX_AXB_VARIANT=52224"), (129, 800, 16, 3, "GLX_AXB_VARIANT=52224 GLX_AXB_S=3")]),
    ("ax", 92278, "f64", 1, "k_ax_dma<MT2,NS2,KC32,NTL1,HOIST1(2:PIPE),W8> S={S}", [
        (1, 32, 16, 1, "GLX_AX_VARIANT=92278"), (6, 32, 32, 1, "GLX_AX_VARIANT=92278"),
        (17, 96, 16, 1, "GLX_AX_VARIANT=92278"), (17, 32, 32, 1, "GLX_AX_VARIANT=92278"),
        (257, 160, 32, 1, "GLX_AX_VARIANT=92278"), (257, 800, 16, 3, "GLX_AX_VARIANT=92278 GLX_AX_S=3")]),
    ("ax", 92278, "f64", 2, "k_ax_dma<MT2,NS2,KC32,NTL1,HOIST1(2:PIPE),W8> S={S}", [
        (1, 32, 16, 1, "GLX_AXB_VARIANT=92278"), (6, 32, 32, 1, "GLX_AXB_VARIANT=92278"),
        (17, 96, 16, 1, "GLX_AXB_VARIANT=92278"), (17, 32, 32, 1, "GLX_AXB_VARIANT=92278"),
        (257, 160, 32, 1, "GLX_AXB_VARIANT=92278"), (257, 800, 16, 3, "GLX_AXB_VARIANT=92278 GLX_AXB_S=3")]),
    # three right-hand sides fit the 160 KiB of LDS at l = 16 only
    ("ax", 92278, "f64", 3, "k_ax_dma<MT2,NS2,KC32,NTL1,HOIST1(2:PIPE),W8> S={S}", [
        (1, 32, 16, 1, "GLX_AXB_VARIANT=92278"), (17, 96, 16, 1, "GLX_AXB_VARIANT=92278"),
        (257, 800, 16, 3, "GLX_AXB_VARIANT=92278 GLX_AXB_S=3")]),
    ("ax", 92268, "f64", 1, "k_ax_dma<MT2,NS2,KC32,NTL0,HOIST1(2:PIPE),W8> S={S}", [
        (1, 32, 16, 1, "GLX_AX_VARIANT=92268"), (6, 32, 32, 1, "GLX_AX_VARIANT=92268"),
        (17, 96, 16, 1, "GLX_AX_VARIANT=92268"), (17, 32, 32, 1, "GLX_AX_VARIANT=92268"),
        (257, 160, 32, 1, "GLX_AX_VARIANT=92268"), (257, 800, 16, 3, "GLX_AX_VARIANT=92268 GLX_AX_S=3")]),
    ("ax", 92268, "f64", 2, "k_ax_dma<MT2,NS2,KC32,NTL0,HOIST1(2:PIPE),W8> S={S}", [
        (1, 32, 16, 1), (6, 32, 32, 1, "GLX_AXB_VARIANT=92268"), (17, 96, 16, 1),
        (17, 32, 32, 1, "GLX_AXB_VARIANT=92268"), (257, 160, 32, 1, "GLX_AXB_VARIANT=92268"),
        (257, 800, 16, 3, "GLX_AXB_S=3"), (33, 96, 16, 1), (33, 1152, 16, 4)]),
    ("ax", 92268, "f64", 3, "k_ax_dma<MT2,NS2,KC32,NTL0,HOIST1(2:PIPE),W8> S={S}", [
        (1, 32, 16, 1, "GLX_AXB_VARIANT=92268"), (17, 96, 16, 1, "GLX_AXB_VARIANT=92268"),
        (257, 800, 16, 3, "GLX_AXB_VARIANT=92268 GLX_AXB_S=3")]),
    ("ax", 92478, "f32", 1, "k_ax_dma<MT2,NS2,KC64,NTL1,HOIST3(2:PIPE),W8> S={S}", [
        (1, 64, 16, 1, "GLX_AX_VARIANT=92478"), (6, 64, 32, 1, "GLX_AX_VARIANT=92478"),
        (17, 192, 16, 1, "GLX_AX_VARIANT=92478"), (17, 64, 32, 1, "GLX_AX_VARIANT=92478"),
        (257, 320, 32, 1, "GLX_AX_VARIANT=92478"), (257, 1600, 16, 3, "GLX_AX_VARIANT=92478 GLX_AX_S=3"),
        (17, 128, 16, 1, "GLX_AX_VARIANT=92478")]),
    ("atr", 3, "f64", 1, "{S}", [
        (6, 64, 16, "k_atr_valu<LB8,VEC1> S=1"), (7, 5, 1, "k_atr_valu<LB1,VEC0> S=1"),
        (6, 66, 3, "k_atr_valu<LB4,VEC1> S=1"), (17, 301, 17, "k_atr_valu<LB8,VEC0> S=1"),
        (5, 64, 32, "k_atr_valu<LB8,VEC1> S=1"), (50, 132, 3, "k_atr_valu<LB4,VEC1> S=3", "GLX_ATR_S=3")]),
    ("atr", 3, "f32", 1, "{S}", [
        (6, 64, 16, "k_atr_valu<LB8,VEC1> S=1"), (7, 5, 1, "k_atr_valu<LB1,VEC0> S=1"),
        (6, 66, 3, "k_atr_valu<LB4,VEC0> S=1"), (17, 301, 17, "k_atr_valu<LB8,VEC0> S=1"),
        (5, 64, 32, "k_atr_valu<LB8,VEC1> S=1"), (50, 132, 3, "k_atr_valu<LB4,VEC1> S=3", "GLX_ATR_S=3")]),
    ("atr", 8, "f64", 1, "k_atr_mfma<WL0,PF8,NTL0> S={S}", [
        (4, 64, 16, 1), (12, 64, 32, 1), (12, 128, 32, 1), (36, 320, 16, 1), (148, 64, 16, 1, "GLX_ATR_S=1"),
        (100, 256, 32, 3, "GLX_ATR_S=3"), (4, 320, 16, 1)]),
    ("atr", 8, "f32", 1, "k_atr_mfma<WL0,PF8,NTL0> S={S}", [
        (4, 64, 16, 1, "GLX_ATR_VARIANT=8"), (12, 64, 32, 1, "GLX_ATR_VARIANT=8"),
        (12, 128, 32, 1, "GLX_ATR_VARIANT=8"), (36, 320, 16, 1, "GLX_ATR_VARIANT=8"),
        (148, 64, 16, 1, "GLX_ATR_VARIANT=8 GLX_ATR_S=1"), (100, 256, 32, 3, "GLX_ATR_VARIANT=8 GLX_ATR_S=3"),
        (4, 320, 16, 1, "GLX_ATR_VARIANT=8")]),
    ("atr", 1008, "f64", 1, "k_atr_mfma<WL0,PF8,NTL1> S={S}", [
        (4, 64, 16, 1, "GLX_ATR_VARIANT=1008"), (12, 64, 32, 1, "GLX_ATR_VARIANT=1008"),
        (12, 128, 32, 1, "GLX_ATR_VARIANT=1008"), (36, 320, 16, 1, "GLX_ATR_VARIANT=1008"),
        (148, 64, 16, 1, "GLX_ATR_VARIANT=1008 GLX_ATR_S=1"), (100, 256, 32, 3, "GLX_ATR_VARIANT=1008 GLX_ATR_S=3"),
        (4, 320, 16, 1, "GLX_ATR_VARIANT=1008")]),
    ("atr", 1008, "f32", 1, "k_atr_mfma<WL0,PF8,NTL1> S={S}", [
        (4, 64, 16, 1), (12, 64, 32, 1), (12, 128, 32, 1), (36, 320, 16, 1), (148, 64, 16, 1, "GLX_ATR_S=1"),
        (100, 256, 32, 3, "GLX_ATR_VARIANT=1008 GLX_ATR_S=3"), (4, 320, 16, 1)]),
    ("atr", 1114, "f64", 1, "k_atr_mfma<WL1,PF4,NTL1> S={S}", [
        (4, 256, 16, 1, "GLX_ATR_VARIANT=1114"), (36, 256, 16, 1, "GLX_ATR_VARIANT=1114"),
        (148, 256, 32, 2, "GLX_ATR_VARIANT=1114"), (100, 256, 32, 3, "GLX_ATR_VARIANT=1114 GLX_ATR_S=3")]),
    ("atr", 1114, "f32", 1, "k_atr_mfma<WL1,PF4,NTL1> S={S}", [
        (4, 256, 16, 1), (36, 256, 16, 1), (148, 256, 32, 2), (100, 256, 32, 3, "GLX_ATR_S=3")]),
    ("atr", 1028, "f64", 1, "k_atr_mfma<WL2,PF8,NTL1> S={S}", [
        (4, 64, 16, 1, "GLX_ATR_VARIANT=1028"), (12, 64, 32, 1, "GLX_ATR_VARIANT=1028"),
        (12, 128, 32, 1, "GLX_ATR_VARIANT=1028"), (36, 320, 16, 1, "GLX_ATR_VARIANT=1028"),
        (148, 64, 16, 1, "GLX_ATR_VARIANT=1028 GLX_ATR_S=1"), (292, 64, 32, 1, "GLX_ATR_VARIANT=1028 GLX_ATR_S=1"),
        (100, 256, 32, 3, "GLX_ATR_VARIANT=1028 GLX_ATR_S=3"), (4, 320, 16, 1, "GLX_ATR_VARIANT=1028")]),
    ("atr", 1028, "f32", 1, "k_atr_mfma<WL2,PF8,NTL1> S={S}", [
        (4, 64, 16, 1, "GLX_ATR_VARIANT=1028"), (12, 64, 32, 1, "GLX_ATR_VARIANT=1028"),
        (12, 128, 32, 1, "GLX_ATR_VARIANT=1028"), (36, 320, 16, 1, "GLX_ATR_VARIANT=1028"),
        (148, 64, 16, 1, "GLX_ATR_VARIANT=1028 GLX_ATR_S=1"), (292, 64, 32, 1, "GLX_ATR_VARIANT=1028 GLX_ATR_S=1"),
        (100, 256, 32, 3, "GLX_ATR_VARIANT=1028 GLX_ATR_S=3"), (4, 320, 16, 1, "GLX_ATR_VARIANT=1028")]),
    ("atr", 38, "f64", 1, "k_atr_mfma<WL3,PF8,NTL0> S={S} (32-column panels)", [
        (4, 64, 16, 1, "GLX_ATR_VARIANT=38"), (12, 64, 32, 1, "GLX_ATR_VARIANT=38"),
        (12, 128, 32, 1, "GLX_ATR_VARIANT=38"), (36, 320, 16, 1, "GLX_ATR_VARIANT=38"),
        (148, 64, 16, 1, "GLX_ATR_VARIANT=38 GLX_ATR_S=1"), (100, 256, 32, 3, "GLX_ATR_VARIANT=38 GLX_ATR_S=3"),
        (4, 320, 16, 1, "GLX_ATR_VARIANT=38"), (36, 128, 16, 3, "GLX_ATR_VARIANT=38 GLX_ATR_S=3")]),
    ("atr", 1038, "f64", 1, "k_atr_mfma<WL3,PF8,NTL1> S={S} (32-column panels)", [
        (4, 64, 16, 1, "GLX_ATR_VARIANT=1038"), (12, 64, 32, 1, "GLX_ATR_VARIANT=1038"),
        (12, 128, 32, 1, "GLX_ATR_VARIANT=1038"), (36, 320, 16, 1, "GLX_ATR_VARIANT=1038"),
        (148, 64, 16, 1, "GLX_ATR_VARIANT=1038 GLX_ATR_S=1"), (100, 256, 32, 3, "GLX_ATR_VARIANT=1038 GLX_ATR_S=3"),
        (4, 320, 16, 1, "GLX_ATR_VARIANT=1038")]),
]

Case = collections.namedtuple("Case", "product code dtype nsrc m n l env plan id")


def parse_env(text):
    env = dict(item.split("=", 1) for item in text.split())
    assert set(env) <= set(KNOBS), text
    return env


def cases(rows=None):
    """The table, one Case per (row, shape); plan is the exact substring of glx_plan_describe."""
    out = []
    for product, code, dtype, nsrc, plan, shapes in (ROWS if rows is None else rows):
        for shape in shapes:
            m, n, l, S = shape[:4]
            env = parse_env(shape[4]) if len(shape) > 4 else {}
            head = "ax%d=" % nsrc if product == "ax" else "atr="
            tag = "%s%d-%d-%s-%dx%dx%d" % (product, nsrc if product == "ax" else 0, code, dtype, m, n, l)
            for k in KNOBS:
                if k in env:
                    tag += "-" + k[4:].replace("VARIANT", "V").replace("_", "") + env[k]
            out.append(Case(product, code, dtype, nsrc, m, n, l, env, head + plan.format(S=S), tag))
    return out


def apply_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
