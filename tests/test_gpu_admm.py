"""The dual ADMM solver on the GPU: its kernels one launch at a time, then whole solves.

Reached through glx_admm_dual_step, glx_gram (glx.kernels) and glx_admm_dual_solve (glx.admm,
gl_ADMM_dual.gl_Admm_dual). References: the formulas of gl_ADMM_dual.py:44-46, 64-67 written below
in NumPy in the next wider type (np.longdouble for f64 inputs, np.float64 for f32 inputs; nothing
imported from glx), float64 NumPy for the Gram matrices, and the reference solver's recorded runs
(tests/golden/admm_dual_*.npz, made by tests/golden/make_admm_golden.py) for whole solves.

1. The row kernel (form 0). Scalars are rounded to T first, as the launcher does: rho, mu and
tau * rho (formed in double, then rounded). eps = T's machine epsilon (u = eps / 2 the unit
roundoff); per row, a_j = |x_j| / rho + |g_j| and N = ||a||_2 >= ||w||. Term by term:
  w    q = x / rho rounds once (u |q|), w = q - g once more (u |w| <= u a_j):
         dw_j <= eps a_j.
  nrm  the l squares (u each), <= 6 additions (2 in a lane, 4 shuffle levels) and the root:
       relative <= (l / 2 + 2) eps on the computed w, plus ||dw|| <= eps N from w itself:
         dn <= (l / 2 + 3) eps N.
  d    max(nrm, mu) is 1-Lipschitz in nrm, so dd <= dn on either side of the switch and across
       it: a row whose norm sits within dn of mu needs no looser bar than its neighbours (both
       branches' bars are this one). Such rows are still counted: at most 4 per case.
  u+   (mu w) / d: two roundings (eps |u|), dw scaled by mu / d <= 1, and dd relative to d:
         du_j <= eps a_j + |u_j| (eps + dn / d).
  r    u+ + g rounds once:  dr_j <= du_j + eps / 2 |r_j|.
  x+   (tau rho) r rounds once, the subtraction once:
         dx_j <= tr dr_j + eps / 2 (tr |r_j| + |x+_j|).
  sum_i ||x+_i||  per row ||dx_i||_2 + (l / 2 + 2) eps ||x+_i|| (as nrm), + CSUM eps64 sum |term|
       for the fp64 accumulation (CSUM = 32 additions deep: a few per thread, 8 levels in the
       workgroup, 12 over the workgroup partials). A thread adds one more row norm in every further
       trip of its workgroup: the several-trip cases take CSUM + trips - 1 (33 at their two trips).
  max |x+|        max_j dx_j (max is 1-Lipschitz in every element).
Each bar is doubled (C = 2) for the second-order terms dropped above. The inputs hold, where n
allows, rows outside the ball, rows strictly inside it (u+ = w up to rounding), an all-zero row, a
row with ||w|| within a few ulp of mu and one NaN row. The NaN turns both sums into NaN, so each
case runs twice: without the NaN row (all the bars above) and with it (every other row
bit-identical to the first run, the row itself NaN, both sums NaN).
A row of l values is held by LPR lanes with EPL values each; the l of test 1 select (LPR, EPL) =
1 (1, 1), 2 (2, 1), 3 (4, 1), 5 and 8 (8, 1), 16 (16, 1), 17 and 32 (16, 2): every instantiation of
k_admm_dual, with a ragged row at LPR 4, LPR 8 and EPL 2, each in one trip of at most 17 workgroups.
test_row_kernel_several_trips runs (l, n) = (1, 131077), (2, 65541), (3, 32771), (8, 16389),
(16, 8200), (17, 8200), (32, 8200): each 5 to 8 rows past the 512 * 256 / LPR rows the capped grid of
512 workgroups takes in one trip, so two trips, the second ragged; u+, x+ and r of the rows on both
sides of the boundary are bit-identical to those of a launch of their own.

2. The fused form (form 1, k_atr_admm) against form 0 on the G it wrote: every bit of u+, x+, r
and of both sums, at the shapes whose plan fuses (asserted from glx_admm_describe). Form 0 is
given m there, so it runs on the panel layout a solve's unfused arm takes (k_admm_dual_panel: the
lanes hold the rows the epilogue's lanes hold, which is what makes the fp64 sums' order, and so
their last bit, the same); the generic row layout of test 1 orders that sum differently. The
panel layout's values are also held to test 1's bars. Beside the planner's own choice, every tile
built for a fused epilogue runs by name (GLX_ATR_VARIANT, with one and two K splits where the tile
takes splits; the tile and S are asserted from the describe string) at (64, 64, 16) and
(192, 256, 32).

3. k_gram against float64 NumPy: the inputs are rounded to T first, the products of doubles are
rounded once each and every entry is a sum of `rows` terms, so
  |gram - ref|_ij <= rows eps64 sum_k |a_ki| |a_kj|   (the bar the issue sets).
rows = 70000 (l = 3 and 32) is past the 65536 rows at which the grid stops growing: 256 workgroups
of 273 or 274 rows each.

4.-6. Whole solves: see each test.

Measured on an MI355X, worst error / bound over all cases (f64, f32); the module prints this table
when its tests are over (pytest -s):
  test 1   u+ 0.255 0.256   r 0.277 0.255   x+ 0.198 0.252   sum ||x+_i|| 0.011 0.029
           max |x+| 0.099 0.080   rows at the switch: 1 per case with n > 3 (the constructed one)
  test 2   (panel layout) u+ 0.016 0.019   r 0.141 0.137   x+ 0.218 0.211
  test 3   gram 0.021 0.030
  test 4   fp64: k identical in all six cases, f_hist within 3.2e-12 relative (the m > n case; the
           others <= 1.1e-13), x within 4.4e-13 of max |x|; fp32: k identical, fval within 2.6e-7.
None is above 1.
"""
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from tile_cases import ROWS as TILE_ROWS

pytestmark = pytest.mark.gpu

RHO, TAU, MU = 1e2, (1 + math.sqrt(5)) * 0.5, 1e-2
C = 2.0
CSUM = 32
MEASURED = {}


def _note(key, ratio):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nworst error / bound:", json.dumps({k: round(v, 4) for k, v in sorted(MEASURED.items())}))


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _wide(dt):
    return np.longdouble if dt == np.float64 else np.float64


def _row_inputs(n, l, dt, seed):
    """x, g of n x l in dt: row kinds by index (0 outside the ball, 1 inside, 2 all-zero, 3 at the
    switch, then random in / out)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, l)).astype(dt)
    g = (rng.standard_normal((n, l)) * 0.05).astype(dt)          # ||w|| ~ 0.05 sqrt(l) > mu: outside
    inside = rng.random(n) < 0.4
    inside[:4] = [False, True, False, False][:n]
    for i in np.nonzero(inside)[0]:                               # ||w|| ~ 0.3 mu: inside
        w = rng.standard_normal(l)
        w *= 0.3 * MU / np.linalg.norm(w)
        g[i] = (rng.standard_normal(l) * 0.05).astype(dt)
        x[i] = ((g[i].astype(np.float64) + w) * RHO).astype(dt)
    if n > 2:
        x[2] = 0
        g[2] = 0
    if n > 3:                                                     # ||w|| = mu (1 + a few eps)
        w = rng.standard_normal(l)
        w *= MU * (1 + 2 * np.finfo(dt).eps) / np.linalg.norm(w)
        g[3] = 0
        x[3] = (w * RHO).astype(dt)
    return x, g


def _row_inputs_large(n, l, dt, seed):
    """_row_inputs for the several-trip cases, drawn in whole arrays (the same row kinds)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, l)).astype(dt)
    g = (rng.standard_normal((n, l)) * 0.05).astype(dt)
    inside = rng.random(n) < 0.4
    inside[:4] = [False, True, False, False]
    w = rng.standard_normal((n, l))
    w *= 0.3 * MU / np.linalg.norm(w, axis=1, keepdims=True)
    x = np.where(inside[:, None], ((g.astype(np.float64) + w) * RHO).astype(dt), x)
    x[2] = 0
    g[2] = 0
    w3 = rng.standard_normal(l)
    w3 *= MU * (1 + 2 * np.finfo(dt).eps) / np.linalg.norm(w3)
    g[3] = 0
    x[3] = (w3 * RHO).astype(dt)
    return x, g


def _row_reference(x, g, dt, csum=CSUM):
    """The row step in the wider type from the T inputs and T-rounded scalars, and the bars. csum:
    the depth of the fp64 accumulation (CSUM at one trip)."""
    W = _wide(dt)
    eps = float(np.finfo(dt).eps)
    rho, mu, tr = W(dt(RHO)), W(dt(MU)), W(dt(TAU * RHO))
    xw, gw = x.astype(W), g.astype(W)
    l = x.shape[1]
    w = xw / rho - gw
    nrm = np.sqrt(np.sum(w * w, axis=1, keepdims=True))
    d = np.maximum(nrm, mu)
    u = mu * w / d
    r = u + gw
    xn = xw - tr * r
    a = np.abs(xw) / rho + np.abs(gw)
    N = np.sqrt(np.sum(a * a, axis=1, keepdims=True))
    dn = (l / 2 + 3) * eps * N
    du = eps * a + np.abs(u) * (eps + dn / d)
    dr = du + eps / 2 * np.abs(r)
    dx = tr * dr + eps / 2 * (tr * np.abs(r) + np.abs(xn))
    xnorm = np.sqrt(np.sum(xn * xn, axis=1))
    dsum = np.sum(np.sqrt(np.sum(dx * dx, axis=1)) + (l / 2 + 2) * eps * xnorm) \
        + csum * np.finfo(np.float64).eps * np.sum(xnorm)
    amb = int(np.sum(np.abs(nrm - mu) <= dn))
    return {"u": u, "r": r, "x": xn, "sum": np.sum(xnorm), "max": np.max(np.abs(xn)),
            "bu": C * du, "br": C * dr, "bx": C * dx, "bsum": C * dsum, "bmax": C * np.max(dx),
            "amb": amb}


def _row_kernel_case(x, g, dt, csum=CSUM):
    """One launch of the row kernel on (x, g) against the wider type, then the same inputs with a
    NaN in the last row; returns the first run's u+, x+, r."""
    torch = _torch()
    from glx import kernels
    n, l = x.shape
    ref = _row_reference(x, g, dt, csum=csum)
    assert ref["amb"] <= 4
    _note("rows at the switch", ref["amb"])
    tag = "f64" if dt == np.float64 else "f32"
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    out = kernels.admm_dual_step(xd, RHO, TAU, MU, G=gd, form=0)
    got = {k: out[k].cpu().numpy() for k in ("u", "x", "r")}
    sums = out["sums"].cpu().numpy()
    for key, bar in (("u", "bu"), ("r", "br"), ("x", "bx")):
        err = np.abs(got[key].astype(_wide(dt)) - ref[key])
        ratio = np.max(err / np.maximum(ref[bar], np.finfo(np.float64).tiny))
        _note(key + " " + tag, ratio)
        assert np.all(err <= ref[bar]), (key, float(ratio))
    if n > 2:   # the all-zero row stays zero
        assert not got["u"][2].any() and not got["x"][2].any() and not got["r"][2].any()
    rs = abs(float(sums[0]) - float(ref["sum"])) / float(ref["bsum"])
    rm = abs(float(sums[1]) - float(ref["max"])) / float(ref["bmax"])
    _note("sum " + tag, rs)
    _note("max " + tag, rm)
    assert rs <= 1 and rm <= 1, (rs, rm)
    # the same inputs with a NaN in the last row: that row NaN, the others untouched, sums NaN
    x2 = x.copy()
    x2[n - 1, l // 2] = np.nan
    out2 = kernels.admm_dual_step(torch.from_numpy(x2).cuda(), RHO, TAU, MU, G=gd, form=0)
    for key in ("u", "x", "r"):
        v = out2[key].cpu().numpy()
        assert np.isnan(v[n - 1]).all()
        assert np.array_equal(v[:n - 1], got[key][:n - 1])
    assert np.isnan(out2["sums"].cpu().numpy()).all()
    return got


# l -> (LPR, EPL) of launch_admm_dual: 1 (1, 1), 2 (2, 1), 3 (4, 1), 5 and 8 (8, 1), 16 (16, 1),
# 17 and 32 (16, 2); 3, 5 and 17 leave lanes or a row's tail elements without a value
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("l", [1, 2, 3, 5, 8, 16, 17, 32])
@pytest.mark.parametrize("n", [1, 15, 64, 130, 257])
def test_row_kernel_against_wider_type(n, l, dt):
    x, g = _row_inputs(n, l, dt, seed=1000 * n + l)
    _row_kernel_case(x, g, dt)


# one n past a single trip of the 512-workgroup grid (512 * 256 / LPR rows) per layout: LPR 1, 2, 4,
# 8, then LPR 16 with EPL 1, a ragged EPL 2 and a full EPL 2; two trips each, the second of 5 to 8 rows
SEVERAL_TRIPS = [(1, 131077), (2, 65541), (3, 32771), (8, 16389), (16, 8200), (17, 8200), (32, 8200)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("l,n", SEVERAL_TRIPS)
def test_row_kernel_several_trips(l, n, dt):
    """Test 1 past one trip (generic layout, m = 1). The sum's bar is test 1's with CSUM + 1 per
    further trip: a thread adds one more row norm to its partial in each. Then the rows on both sides
    of the trip boundary run again as an input of their own, in one trip: u+, x+ and r of a row depend
    on neither n nor the trip, so they come back bit for bit (the wrapper pre-fills them with NaN)."""
    torch = _torch()
    from glx import kernels
    lpr = 1
    while lpr < min(l, 16):
        lpr *= 2
    per_trip = 512 * 256 // lpr
    trips = -(-n // per_trip)
    assert trips == 2 and 0 < n - per_trip < 256 // lpr
    x, g = _row_inputs_large(n, l, dt, seed=1000 * n + l)
    got = _row_kernel_case(x, g, dt, csum=CSUM + trips - 1)
    rows = slice(per_trip - 251, n)
    part = kernels.admm_dual_step(torch.from_numpy(x[rows].copy()).cuda(), RHO, TAU, MU,
                                  G=torch.from_numpy(g[rows].copy()).cuda(), form=0)
    for key in ("u", "x", "r"):
        assert np.array_equal(_bits(part[key].cpu().numpy()), _bits(got[key][rows])), key


FUSED_CASES = [(64, 64, 16, np.float64, None, None), (128, 128, 32, np.float64, None, None),
               (192, 256, 32, np.float64, None, None), (128, 256, 32, np.float32, None, None),
               (64, 64, 16, np.float64, "2", None)]
FUSED_IDS = ["64x64x16", "128x128x32", "192x256x32", "f32_128x256x32", "64x64x16_S2"]
# every fused tile by name (GLX_ATR_VARIANT) with the K splits it takes under an epilogue, at one
# panel with NT = 1 and at several panels with NT = 2 and m not a power of two: four-wave,
# eight-wave (1028) and 32-column (38, 1038) row ownership, split and not
FUSED_TILES = [(8, (np.float64,), (1, 2)), (1008, (np.float64, np.float32), (1, 2)),
               (1028, (np.float64, np.float32), (1, 2)), (38, (np.float64,), (1,)), (1038, (np.float64,), (1,))]
for _shape in ((64, 64, 16), (192, 256, 32)):
    for _tile, _dts, _Ss in FUSED_TILES:
        for _dt in _dts:
            for _S in _Ss:
                FUSED_CASES.append(_shape + (_dt, str(_S), _tile))
                FUSED_IDS.append("%s%dx%dx%d_t%d_S%d" % (("f32_" if _dt == np.float32 else "",) + _shape + (_tile, _S)))
ATR_NAMES = {row[1]: row[4] for row in TILE_ROWS if row[0] == "atr"}   # tile -> its name in a describe string


@pytest.mark.parametrize("m,n,l,dt,splits,tile", FUSED_CASES, ids=FUSED_IDS)
def test_fused_form_is_bit_identical(m, n, l, dt, splits, tile, monkeypatch):
    torch = _torch()
    from glx import _lib, kernels
    if splits is not None:
        monkeypatch.setenv("GLX_ATR_S", splits)
    if tile is not None:
        monkeypatch.setenv("GLX_ATR_VARIANT", str(tile))
    gdt = _lib.GLX_F64 if dt == np.float64 else _lib.GLX_F32
    d = _lib.admm_describe(gdt, m, n, l)
    assert "projection=fused" in d, d
    if splits is not None:
        assert "S=%s" % splits in d.split("A^T z=")[1], d
    if tile is not None:   # the named tile and S were planned
        assert d.split("A^T z=")[1].split(";")[0] == ATR_NAMES[tile].format(S=splits), d
    rng = np.random.default_rng(m + n + l)
    A = torch.from_numpy(rng.standard_normal((m, n)).astype(dt)).cuda()
    Z = torch.from_numpy((rng.standard_normal((m, l)) * 0.01).astype(dt)).cuda()
    x, _ = _row_inputs(n, l, dt, seed=7)
    xd = torch.from_numpy(x).cuda()
    f1 = kernels.admm_dual_step(xd, RHO, TAU, MU, A=A, Z=Z, form=1)
    # G itself: A^T Z within a dot product's bar of float64 NumPy
    Gref = A.cpu().numpy().astype(np.float64).T @ Z.cpu().numpy().astype(np.float64)
    Gabs = np.abs(A.cpu().numpy().astype(np.float64)).T @ np.abs(Z.cpu().numpy().astype(np.float64))
    assert np.all(np.abs(f1["G"].cpu().numpy() - Gref) <= (m + 2) * float(np.finfo(dt).eps) * Gabs)
    f0 = kernels.admm_dual_step(xd, RHO, TAU, MU, G=f1["G"], form=0, m=m)
    it = torch.int64 if dt == np.float64 else torch.int32
    for key in ("u", "x", "r"):
        assert torch.equal(f1[key].view(it), f0[key].view(it)), key
    assert torch.equal(f1["sums"].view(torch.int64), f0["sums"].view(torch.int64))
    # and the panel layout's arithmetic against the wider type, under test 1's bars
    ref = _row_reference(x, f1["G"].cpu().numpy(), dt)
    tag = "panel f64" if dt == np.float64 else "panel f32"
    for key, bar in (("u", "bu"), ("r", "br"), ("x", "bx")):
        err = np.abs(f1[key].cpu().numpy().astype(_wide(dt)) - ref[key])
        _note(key + " " + tag, np.max(err / np.maximum(ref[bar], np.finfo(np.float64).tiny)))
        assert np.all(err <= ref[bar]), key
    sums = f1["sums"].cpu().numpy()
    assert abs(float(sums[0]) - float(ref["sum"])) <= float(ref["bsum"])
    assert abs(float(sums[1]) - float(ref["max"])) <= float(ref["bmax"])


def test_fused_form_refuses_small_l():
    torch = _torch()
    from glx import _lib, kernels
    A = torch.zeros((64, 128), dtype=torch.float64, device="cuda")
    Z = torch.zeros((64, 2), dtype=torch.float64, device="cuda")
    x = torch.zeros((128, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.GlxError) as e:
        kernels.admm_dual_step(x, RHO, TAU, MU, A=A, Z=Z, form=1)
    assert e.value.code == 1   # GLX_E_INVALID


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
# (70000 rows: past 65536 the grid stays at 256 workgroups, which own 273 or 274 rows each)
@pytest.mark.parametrize("rows,l", [(r, l) for r in (1, 63, 1000, 4097) for l in (1, 2, 3, 16, 32)]
                         + [(70000, 3), (70000, 32)])
def test_gram(rows, l, dt):
    torch = _torch()
    from glx import kernels
    rng = np.random.default_rng(rows * 37 + l)
    R = (rng.standard_normal((rows, l)) * rng.choice([1e-3, 1.0, 30.0], size=(rows, 1))).astype(dt)
    Rd = torch.from_numpy(R).cuda()
    g1 = kernels.gram(Rd)
    g2 = kernels.gram(Rd)
    assert torch.equal(g1.view(torch.int64), g2.view(torch.int64))
    r64 = R.astype(np.float64)
    ref = r64.T @ r64
    bar = rows * np.finfo(np.float64).eps * (np.abs(r64).T @ np.abs(r64))
    err = np.abs(g1.cpu().numpy() - ref)
    _note("gram " + ("f64" if dt == np.float64 else "f32"), np.max(err / bar))
    assert np.all(err <= bar)
    assert np.array_equal(g1.cpu().numpy(), g1.cpu().numpy().T)   # the stop rule's Jacobi sweep reads it as symmetric


# ---------------------------------------------------------------------------------------------
# whole solves
# ---------------------------------------------------------------------------------------------
with open(os.path.join(GOLDEN, "admm_index.json")) as _fh:
    INDEX = json.load(_fh)
CASES = sorted(INDEX)


def _case(name):
    from test_admm_cpu import load_case
    return load_case(name)


@pytest.mark.parametrize("name", CASES)
def test_solve_f64_against_reference(name):
    """k identical; fval, f_hist, f_hist_best within 1e-8 relative (the project's fp64 parity bar;
    the CPU restatement sits at <= 1.2e-12); x within 1e-6 of max |x|."""
    _torch()
    from gl_ADMM_dual import gl_Admm_dual
    meta, arrs, A, b, x0, mu = _case(name)
    x, k, out = gl_Admm_dual(x0, A, b, mu, {})
    assert k == int(arrs["k"])
    fh, fb = np.asarray(out["f_hist"]), np.asarray(out["f_hist_best"])
    assert len(fh) == k and len(fb) == k
    print(name, "k", k, "fval rel", abs(float(out["fval"]) - float(arrs["fval"])) / float(arrs["fval"]),
          "f_hist rel", float(np.max(np.abs(fh - arrs["f_hist"]) / np.abs(arrs["f_hist"]))),
          "x", float(np.max(np.abs(x - arrs["x"])) / np.max(np.abs(arrs["x"]))))
    assert abs(float(out["fval"]) - float(arrs["fval"])) <= 1e-8 * abs(float(arrs["fval"]))
    assert np.max(np.abs(fh - arrs["f_hist"]) / np.abs(arrs["f_hist"])) <= 1e-8
    assert np.max(np.abs(fb - arrs["f_hist_best"]) / np.abs(arrs["f_hist_best"])) <= 1e-8
    assert np.max(np.abs(x - arrs["x"])) <= 1e-6 * np.max(np.abs(arrs["x"]))
    assert out["glx"]["syncs"] == k and out["glx"]["k_calls"] == k and out["glx"]["atr_calls"] == k
    assert out["glx"]["ax_calls"] == k + 1
    assert out["glx"]["fused"] == ("projection=fused" in out["glx"]["plan"])


@pytest.mark.parametrize("name", [c for c in CASES if INDEX[c]["m"] < INDEX[c]["n"]])
def test_solve_f32_against_reference(name):
    """fp32 on the m < n cases: k identical, fval within 1e-4 relative (the project's fp32 bar; the
    CPU emulation sits at <= 2.7e-7). The m > n case is not run in fp32: K cast to fp32 costs
    1.2e-3 there."""
    _torch()
    from gl_ADMM_dual import gl_Admm_dual
    meta, arrs, A, b, x0, mu = _case(name)
    x, k, out = gl_Admm_dual(x0.astype(np.float32), A.astype(np.float32), b.astype(np.float32), mu, {})
    print(name, "k", k, "fval rel", abs(float(out["fval"]) - float(arrs["fval"])) / float(arrs["fval"]))
    assert x.dtype == np.float32
    assert k == int(arrs["k"])
    assert abs(float(out["fval"]) - float(arrs["fval"])) <= 1e-4 * abs(float(arrs["fval"]))


def test_fused_against_unfused_and_overrides():
    """(128, 256, 32) fp64: fused = 1 and fused = 2 give the same bits of x, f_hist and k, and so
    does a repeat; the maxit, thres, rho, tau, converge_len overrides reach the solver."""
    _torch()
    from glx import admm
    meta, arrs, A, b, x0, mu = _case("admm_dual_128x256x32")
    x1, k1, o1 = admm.solve(x0, A, b, mu, {"fused": 1})
    x2, k2, o2 = admm.solve(x0, A, b, mu, {"fused": 2})
    x3, k3, o3 = admm.solve(x0, A, b, mu, {"fused": 1})
    assert o1["glx"]["fused"] and not o2["glx"]["fused"]
    assert k1 == k2 == k3 == int(arrs["k"])
    assert np.array_equal(x1, x2) and np.array_equal(x1, x3)
    assert o1["f_hist"] == o2["f_hist"] == o3["f_hist"]
    # a short maxit ends with k = maxit
    xs, ks, os_ = admm.solve(x0, A, b, mu, {"maxit": 3})
    assert ks == 3 and len(os_["f_hist"]) == 3 and os_["f_hist"] == o1["f_hist"][:3]
    assert os_["fval"] == os_["f_hist"][-1]
    # converge_len and thres: with a huge thres every iteration counts, so k = converge_len
    _, kc, _ = admm.solve(x0, A, b, mu, {"thres": 1e30, "converge_len": 5})
    assert kc == 5
    # rho and tau change the iterates (and rho the factor K)
    _, _, orho = admm.solve(x0, A, b, mu, {"maxit": 3, "rho": 50.0})
    _, _, otau = admm.solve(x0, A, b, mu, {"maxit": 3, "tau": 1.0})
    assert orho["f_hist"] != os_["f_hist"] and otau["f_hist"] != os_["f_hist"]
    import admm_ref
    for o, got in (({"maxit": 3, "rho": 50.0}, orho), ({"maxit": 3, "tau": 1.0}, otau)):
        _, _, want = admm_ref.gl_admm_dual(x0, A, b, mu, o)
        assert np.allclose(got["f_hist"], want["f_hist"], rtol=1e-8, atol=0)
    # maxit = 0: no iteration, the objective of x0
    x0c, k0, o0 = admm.solve(x0, A, b, mu, {"maxit": 0})
    assert k0 == 0 and o0["f_hist"] == [] and np.array_equal(x0c, x0)
    f0 = 0.5 * np.sum((A @ x0 - b) ** 2) + mu * np.sum(np.linalg.norm(x0, axis=1))
    assert abs(float(o0["fval"]) - f0) <= 1e-10 * f0


def test_drop_in_module_contract():
    """gl_ADMM_dual.gl_Admm_dual on the default instance with NumPy arrays: NumPy out, x0 and the
    caller's opts untouched, the reference's keys."""
    torch = _torch()
    from gl_ADMM_dual import gl_Admm_dual
    meta, arrs, A, b, x0, mu = _case("admm_dual_256x512x2")
    x0_before = x0.copy()
    opts = {"maxit": 10, "not_an_option": 1}
    opts_before = dict(opts)
    x, k, out = gl_Admm_dual(x0, A, b, mu, opts)
    assert isinstance(x, np.ndarray) and x.dtype == np.float64 and x.shape == x0.shape
    assert isinstance(k, int) and k == 10
    assert np.array_equal(x0, x0_before) and opts == opts_before
    assert {"tt", "fval", "f_hist", "f_hist_best", "glx"} <= set(out)
    assert out["tt"] >= out["glx"]["setup_s"] > 0
    assert np.allclose(out["f_hist"], arrs["f_hist"][:10], rtol=1e-8, atol=0)
    # torch in, torch out
    xt, kt, outt = gl_Admm_dual(torch.from_numpy(x0).cuda(), torch.from_numpy(A).cuda(),
                                torch.from_numpy(b).cuda(), mu, opts)
    assert isinstance(xt, torch.Tensor) and kt == 10 and np.array_equal(xt.cpu().numpy(), x)
