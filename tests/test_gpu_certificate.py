"""The optimality certificate on the GPU: its row kernels one launch at a time, then whole
certificates, the Python interface and the driver's --certify columns.

Reached through glx_certificate_step (glx.kernels.certificate_step) and glx_certificate
(glx.certificate, glx.mu_max, glx.certificate.record). Reference: tests/certificate_ref.py in the
next wider type (np.longdouble for f64 inputs, np.float64 for f32 inputs); float64 NumPy for G.

Notation. eps = T's machine epsilon, u = eps / 2, eps64 the accumulator's. A row of l values is held
by LPR lanes with EPL values each (l <= 8: LPR = the power of two >= l, EPL = 1; above: LPR = 16,
EPL = ceil(l / 16); the panel layout of the fused form is LPR 16, EPL l / 16).

1. The row kernel (form 0) on a given G. mu is rounded to T first, as the launcher does. Term by
term, per row i:
  norms  ||g_i|| and ||x_i|| from exact inputs: the squares round once (u), a sum path has
         EPL - 1 additions in the lane and log2 LPR shuffle levels, the root halves the relative
         error of its argument and rounds once:
           relative <= RN = (EPL + log2 LPR + 2) / 4 eps.
  kkt, x_i = 0   d = ||g_i|| - mu rounds once, max(d, 0) is 1-Lipschitz:
           dkkt_i <= RN ||g_i|| + u | ||g_i|| - mu |
         on either side of the switch ||g_i|| = mu and across it, so rows within a few ulp of mu
         need no looser bar.
  kkt, x_i != 0  t_j = (mu x_j) / ||x_i||: two roundings and the norm's error, dt_j <= |t_j| (eps + RN);
         k_j = g_j + t_j rounds once, dk_j <= dg_j + dt_j + u |k_j| (dg = 0 here, the product's bar in
         test 3); then the norm of k as above:
           dkkt_i <= ||dk_i||_2 + RN ||k_i||.
         Which branch a row takes is decided by ||x_i|| == 0, exact for an all-zero row and for the
         O(1) entries used here (no underflow), so no row is ambiguous.
  sum_i ||x_i||   sum_i RN ||x_i|| + CSUM eps64 sum_i ||x_i|| for the fp64 accumulation (CSUM = 32
         additions deep: a few per thread, 8 levels in the workgroup, 12 over the partials). A thread
         adds one more term in every further trip of its workgroup: the several-trip cases take
         CSUM + trips - 1 (33 at their two trips).
  max_i ||g_i||   max_i (||dg_i||_2 + RN ||g_i||): max is 1-Lipschitz in every element.
  max_i kkt_i     max_i dkkt_i, likewise.
  sum_i kkt_i^2   sum_i (2 kkt_i dkkt_i + dkkt_i^2) + (CSUM + 1) eps64 sum_i kkt_i^2 (the square is
         formed in double and rounds once).
  nonzero rows    exact.
Each bar is doubled (C = 2) for the second-order terms dropped above. The inputs hold, where n
allows: a nonzero random row, a zero row with ||g|| above mu, an all-zero row (x = g = 0), zero rows
with ||g|| = mu (1 +- 2 eps), a zero row with ||g|| = 0.3 mu, a nonzero row that nearly satisfies
its KKT condition (g = -mu x / ||x|| + 1e-3 mu noise), then random rows of those kinds. Each case
runs twice: as built, and with one NaN in the last row of x. ||g_i|| does not read x, so the row
norms and max_i ||g_i|| of the second run are bit-identical to the first; the three sums and the
max that the NaN row feeds (sum ||x_i||, max kkt, sum kkt^2, and the row count) are NaN.
The l of test 1 select (LPR, EPL) = 1 (1, 1), 2 (2, 1), 3 (4, 1), 5 and 8 (8, 1), 16 (16, 1),
32 (16, 2), 33 (16, 3), 64 (16, 4), 72 (16, 5), 88 (16, 6), 104 (16, 7), 128 (16, 8): every
instantiation of k_cert_row, each in one trip of at most 17 workgroups. test_row_kernel_several_trips
runs (l, n) = (1, 131077), (2, 65541), (3, 32771), (8, 16389), (16, 8200), (128, 8200): LPR 1, 2, 4, 8
and LPR 16 at EPL 1 and 8, each 5 to 8 rows past the 512 * 256 / LPR rows the capped grid of 512
workgroups takes in one trip, so two trips, the second ragged; the norms of the rows on both sides
of the boundary are bit-identical to those of a launch of their own.

2. Fused against unfused at the shapes whose plan fuses (asserted from glx_certificate_describe):
the five sums and the row norms of form 1 (k_atr_cert) and of form 0 on the G it wrote, given m
(k_cert_panel), bit for bit; the whole record and row norms of glx.certificate with fused = 1 and
fused = 2, bit for bit; G within (m + 2) eps |A|^T |r| of float64 NumPy (the bar the issue sets).
Beside the planner's own choice, every tile built for a fused epilogue runs by name
(GLX_ATR_VARIANT, with one and two K splits where the tile takes splits; the tile and S are asserted
from the describe string) at (64, 64, 16) and (192, 256, 32).

3. Whole certificates. The products' bars, elementwise: dr = (n + 2) eps (|A| |x| + |b|) for
r = A x - b (the issue's), dg = (m + 2) eps |A|^T |r| + |A|^T dr for g = A^T r. Then
  ||r||^2   sum (2 |r| dr + dr^2) + (CSUM + 1) eps64 ||r||^2
  <r, b>    sum |b| dr + (CSUM + 1) eps64 sum |r b|
  sum ||x_i||, gmax, kkt_max, sum kkt^2   as in test 1 with dg above.
The gap is G(rr, rb, sx, s) = 1/2 (1 + s^2) rr + s rb + mu sx with s = min(1, mu / gmax). To first
order
  dgap <= 1/2 (1 + s^2) d_rr + s d_rb + mu d_sx + |s rr + rb| ds + 4 eps64 (1/2 (1 + s^2) rr + |s rb| + mu sx),
where ds = min(1, mu / (gmax - d_gmax)) - min(1, mu / (gmax + d_gmax)) is the whole interval of s
(0 while gmax + d_gmax <= mu; no special case at the switch), and the last term is the host's
composition in double. Bars doubled as in test 1. mu_max = gmax at x = 0, where r = -b is exact:
its bar is gmax's with dr = 0.

Measured on an MI355X, worst error / bound over all cases (f64, f32); the module prints this table
when its tests are over (pytest -s):
  test 1   sum ||x_i|| 0.014 0.18   max ||g_i|| 0.32 0.17   max kkt 0.25 0.25   sum kkt^2 0.013 0.22
           row norms 0.50 0.43
  test 2   (panel layout) sum ||x_i|| 0.012 0.022   max ||g_i|| <1e-4 0.085   max kkt 0.15 0.090
           sum kkt^2 0.013 0.028   G 0.024 0.011; forms 0 / 1 and fused = 1 / 2 bit-identical
  test 3   ||r||^2 1e-4 1e-4   <r, b> 2e-4 <1e-4   sum ||x_i|| <1e-4 8e-4   gmax 1e-4 1e-4
           kkt_max 2e-4 1e-4   sum kkt^2 <1e-4 <1e-4   gap <1e-4 1e-4   mu_max <1e-4 (its bars carry
           the worst-case dot-product terms); at x*: gap 1.14e-11 = 1.87e-11 of primal, kkt_max 2.5e-13;
           at the ALM results gap / primal 2.0e-4 to 1.0e-3
None exceeds 1.
"""
import io
import json
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
from tile_cases import ROWS as TILE_ROWS

import certificate_ref as cref

pytestmark = pytest.mark.gpu

MU = 1e-2
C = 2.0
CSUM = 32
EPS64 = float(np.finfo(np.float64).eps)
TINY = float(np.finfo(np.float64).tiny)
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


def _tag(dt):
    return "f64" if dt == np.float64 else "f32"


def _rn(l, dt):
    """RN: the relative bar of a row norm of l values (docstring, "norms")."""
    lpr = 1
    while lpr < min(l, 16):
        lpr *= 2
    epl = -(-l // lpr)
    return (epl + math.log2(lpr) + 2) / 4 * float(np.finfo(dt).eps)


def _row_bars(x, g, mu, dt, dg=None, csum=CSUM):
    """The row terms of x, g (T values) in the wider type with mu = T(mu), and their bars (already
    doubled). dg: the elementwise bar of g (None: g is exact). csum: the depth of the fp64
    accumulation (CSUM at one trip)."""
    W = _wide(dt)
    eps = float(np.finfo(dt).eps)
    l = x.shape[1]
    RN = _rn(l, dt)
    muw = W(dt(mu))
    ref = cref.row_terms(x.astype(W), g.astype(W), muw)
    xn, gn, kkt = (ref[k].astype(np.float64) for k in ("xnorm", "gnorm", "kkt"))
    dgv = np.zeros(x.shape) if dg is None else np.asarray(dg, dtype=np.float64)
    dgn = np.sqrt(np.sum(dgv * dgv, axis=1)) + RN * gn
    nz = xn != 0
    safe = np.where(nz, xn, 1.0)[:, None]
    t = float(muw) * x.astype(np.float64) / safe
    k = g.astype(np.float64) + t
    dk = dgv + np.abs(t) * (eps + RN) + eps / 2 * np.abs(k)
    dk_nz = np.sqrt(np.sum(dk * dk, axis=1)) + RN * np.sqrt(np.sum(k * k, axis=1))
    dk_z = dgn + eps / 2 * np.abs(gn - float(muw))
    dkkt = np.where(nz, dk_nz, dk_z)
    bars = {
        "sum_xnorm": C * (RN + csum * EPS64) * np.sum(xn),
        "gmax": C * np.max(dgn),
        "kkt_max": C * np.max(dkkt),
        "kkt_sq": C * (np.sum(2 * kkt * dkkt + dkkt * dkkt) + (csum + 1) * EPS64 * np.sum(kkt * kkt)),
        "gnorm": C * dgn,
    }
    return ref, bars


def _check_sums(sums, ref, bars, tag, where):
    names = ("sum_xnorm", "gmax", "kkt_max", "kkt_sq")
    worst = {}
    for i, name in enumerate(names):
        err = abs(float(sums[i]) - float(ref["sums"][i]))
        ratio = err / max(float(bars[name]), TINY)
        print("%s %s %s: got %.17g ref %.17g err %.3e bar %.3e" % (where, tag, name, float(sums[i]),
                                                                  float(ref["sums"][i]), err, float(bars[name])))
        _note("%s %s %s" % (where, name, tag), ratio)
        worst[name] = ratio
    assert all(v <= 1 for v in worst.values()), worst
    assert float(sums[4]) == float(ref["sums"][4])


def _row_inputs(n, l, dt, seed):
    """x, g of n x l in dt: row kinds by index (docstring), then random kinds."""
    rng = np.random.default_rng(seed)
    eps = float(np.finfo(dt).eps)
    mu = float(dt(MU))

    def unit():
        w = rng.standard_normal(l)
        return w / np.linalg.norm(w)

    x = np.zeros((n, l))
    g = np.zeros((n, l))
    kinds = [0, 1, 2, 3, 4, 5, 6] + list(rng.integers(0, 7, size=max(0, n - 7)))
    for i in range(n):
        kind = kinds[i]
        if kind == 0:                       # nonzero row, g unrelated
            x[i] = rng.standard_normal(l)
            g[i] = rng.standard_normal(l) * 0.05
        elif kind == 1:                     # zero row, ||g|| above mu
            g[i] = unit() * mu * (1.5 + rng.random() * 5)
        elif kind == 2:                     # all-zero row
            pass
        elif kind == 3:                     # zero row, ||g|| a few ulp above mu
            g[i] = unit() * mu * (1 + 2 * eps)
        elif kind == 4:                     # zero row, ||g|| a few ulp below mu
            g[i] = unit() * mu * (1 - 2 * eps)
        elif kind == 5:                     # zero row well inside
            g[i] = unit() * mu * 0.3
        else:                               # nonzero row close to its KKT condition
            x[i] = rng.standard_normal(l)
            g[i] = -mu * x[i] / np.linalg.norm(x[i]) + 1e-3 * mu * rng.standard_normal(l)
    return x.astype(dt), g.astype(dt)


def _row_inputs_large(n, l, dt, seed):
    """_row_inputs' seven row kinds for the several-trip cases, drawn in whole arrays: the first seven
    rows hold one kind each, the rest random kinds. The random values differ from row to row, so no
    two rows agree except the all-zero ones."""
    rng = np.random.default_rng(seed)
    eps = float(np.finfo(dt).eps)
    mu = float(dt(MU))
    kinds = np.concatenate([np.arange(7), rng.integers(0, 7, size=max(0, n - 7))])[:n, None]
    w = rng.standard_normal((n, l))
    unit = w / np.linalg.norm(w, axis=1, keepdims=True)
    xr = rng.standard_normal((n, l))
    far = 1.5 + rng.random((n, 1)) * 5
    noise = rng.standard_normal((n, l))
    x = np.where((kinds == 0) | (kinds == 6), xr, 0.0)
    near = -mu * xr / np.linalg.norm(xr, axis=1, keepdims=True) + 1e-3 * mu * noise
    g = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3, kinds == 4, kinds == 5],
                  [noise * 0.05, unit * mu * far, 0.0 * unit, unit * mu * (1 + 2 * eps), unit * mu * (1 - 2 * eps),
                   unit * mu * 0.3], near)
    return x.astype(dt), g.astype(dt)


def _row_kernel_case(x, g, dt, csum=CSUM):
    """One launch of the row kernel on (x, g) against the wider type, then the same inputs with a
    NaN in the last row of x; returns the first run's row norms."""
    torch = _torch()
    from glx import kernels
    n, l = x.shape
    ref, bars = _row_bars(x, g, MU, dt, csum=csum)
    tag = _tag(dt)
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    out = kernels.certificate_step(xd, MU, G=gd, form=0)
    sums = out["sums"].cpu().numpy()
    rn = out["row_norms"].cpu().numpy()
    _check_sums(sums, ref, bars, tag, "test 1")
    err = np.abs(rn - ref["gnorm"].astype(np.float64))
    ratio = float(np.max(err / np.maximum(bars["gnorm"], TINY)))
    _note("test 1 row norms " + tag, ratio)
    assert np.all(err <= bars["gnorm"]), ratio
    assert np.array_equal(out["G"].cpu().numpy(), g)       # form 0 leaves the given G alone
    # the same inputs with a NaN in the last row of x
    x2 = x.copy()
    x2[n - 1, l // 2] = np.nan
    out2 = kernels.certificate_step(torch.from_numpy(x2).cuda(), MU, G=gd, form=0)
    s2 = out2["sums"].cpu().numpy()
    assert np.isnan(s2[[0, 2, 3, 4]]).all(), s2
    assert s2[1] == sums[1]
    assert np.array_equal(out2["row_norms"].cpu().numpy(), rn)
    return rn


# l -> (LPR, EPL) of cert_dispatch_row: 1 (1, 1), 2 (2, 1), 3 (4, 1), 5 and 8 (8, 1), 16 (16, 1),
# 32 (16, 2), 33 (16, 3), 64 (16, 4), 72 (16, 5), 88 (16, 6), 104 (16, 7), 128 (16, 8)
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("l", [1, 2, 3, 5, 8, 16, 32, 33, 64, 72, 88, 104, 128])
@pytest.mark.parametrize("n", [1, 15, 64, 130, 257])
def test_row_kernel_against_wider_type(n, l, dt):
    x, g = _row_inputs(n, l, dt, seed=1000 * n + l)
    _row_kernel_case(x, g, dt)


# one n past a single trip of the 512-workgroup grid (512 * 256 / LPR rows) per lanes-per-row layout:
# LPR 1, 2, 4, 8, then LPR 16 with EPL 1 and EPL 8; two trips each, the second of 5 to 8 rows
SEVERAL_TRIPS = [(1, 131077), (2, 65541), (3, 32771), (8, 16389), (16, 8200), (128, 8200)]


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("l,n", SEVERAL_TRIPS)
def test_row_kernel_several_trips(l, n, dt):
    """Test 1 past one trip (generic layout, m = 1). The bars are test 1's with CSUM + 1 per further
    trip: a thread adds one more term to its partial sums in each. Then the rows on both sides of the
    trip boundary run again as an input of their own, in one trip: a row's norm depends on neither n
    nor the trip, so it comes back bit for bit (the wrapper pre-fills the norms with NaN)."""
    torch = _torch()
    from glx import kernels
    lpr = 1
    while lpr < min(l, 16):
        lpr *= 2
    per_trip = 512 * 256 // lpr
    trips = -(-n // per_trip)
    assert trips == 2 and 0 < n - per_trip < 256 // lpr
    x, g = _row_inputs_large(n, l, dt, seed=1000 * n + l)
    rn = _row_kernel_case(x, g, dt, csum=CSUM + trips - 1)
    rows = slice(per_trip - 251, n)
    part = kernels.certificate_step(torch.from_numpy(x[rows].copy()).cuda(), MU,
                                    G=torch.from_numpy(g[rows].copy()).cuda(), form=0)
    assert np.array_equal(part["row_norms"].cpu().numpy().view(np.uint64), rn[rows].view(np.uint64))


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
    import glx
    from glx import _lib, kernels
    from glx.certificate import record
    if splits is not None:
        monkeypatch.setenv("GLX_ATR_S", splits)
    if tile is not None:
        monkeypatch.setenv("GLX_ATR_VARIANT", str(tile))
    gdt = _lib.GLX_F64 if dt == np.float64 else _lib.GLX_F32
    d = _lib.certificate_describe(gdt, m, n, l)
    assert "rows=fused" in d, d
    if splits is not None:
        assert "S=%s" % splits in d.split("A^T r=")[1], d
    if tile is not None:   # the named tile and S were planned
        assert d.split("A^T r=")[1].split(";")[0] == ATR_NAMES[tile].format(S=splits), d
    rng = np.random.default_rng(m + n + l)
    A = rng.standard_normal((m, n)).astype(dt)
    r = rng.standard_normal((m, l)).astype(dt)
    x = rng.standard_normal((n, l)).astype(dt)
    x[::3] = 0
    Ad, rd, xd = (torch.from_numpy(a).cuda() for a in (A, r, x))
    f1 = kernels.certificate_step(xd, MU, form=1, A=Ad, Z=rd)
    f0 = kernels.certificate_step(xd, MU, G=f1["G"], form=0, m=m)
    assert np.array_equal(f1["sums"].cpu().numpy(), f0["sums"].cpu().numpy())
    assert np.array_equal(f1["row_norms"].cpu().numpy(), f0["row_norms"].cpu().numpy())
    G = f1["G"].cpu().numpy().astype(np.float64)
    A64, r64 = A.astype(np.float64), r.astype(np.float64)
    bar = (m + 2) * float(np.finfo(dt).eps) * (np.abs(A64).T @ np.abs(r64))
    err = np.abs(G - A64.T @ r64)
    _note("test 2 G " + _tag(dt), np.max(err / bar))
    assert np.all(err <= bar), float(np.max(err / bar))
    # the panel layout's sums are held to test 1's bars, on the G the product wrote
    ref, bars = _row_bars(x, f1["G"].cpu().numpy(), MU, dt)
    _check_sums(f0["sums"].cpu().numpy(), ref, bars, _tag(dt), "test 2")
    # the whole certificate, fused = 1 against fused = 2
    b = rng.standard_normal((m, l)).astype(dt)
    c1 = glx.certificate(x, A, b, MU, fused=1, row_norms=True)
    c2 = glx.certificate(x, A, b, MU, fused=2, row_norms=True)
    assert c1["fused"] is True and c2["fused"] is False
    assert "fused" in c1["plan"] and "row kernel" in c2["plan"]
    for key in ("primal", "dual", "gap", "rel_gap", "scale", "gmax", "kkt_max", "kkt_fro", "nonzero_rows"):
        assert c1[key] == c2[key], key
    assert np.array_equal(c1["row_norms"], c2["row_norms"])
    assert np.array_equal(record(x, A, b, MU, fused=1)[:7], record(x, A, b, MU, fused=2)[:7])


def test_fused_form_is_refused_at_l2():
    torch = _torch()
    from glx import GlxError, kernels
    A = torch.zeros((64, 64), dtype=torch.float64, device="cuda")
    Z = torch.zeros((64, 2), dtype=torch.float64, device="cuda")
    x = torch.zeros((64, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(GlxError, match="fused"):
        kernels.certificate_step(x, MU, form=1, A=A, Z=Z)


# ---- 3. whole certificates ----
def _cert_bars(x, A, b, mu, dt, zero_x=False):
    """certificate_ref in the wider type at T inputs, and the bars of test 3 (doubled)."""
    W = _wide(dt)
    eps = float(np.finfo(dt).eps)
    m, n = A.shape
    muT = float(dt(mu))
    ref = cref.certificate(x.astype(W), A.astype(W), b.astype(W), W(muT))
    A64, x64, b64 = (np.abs(a.astype(np.float64)) for a in (A, x, b))
    r64 = np.abs(ref["r"].astype(np.float64))
    dr = np.zeros(b.shape) if zero_x else (n + 2) * eps * (A64 @ x64 + b64)
    dg = (m + 2) * eps * (A64.T @ r64) + A64.T @ dr
    g_T = ref["g"].astype(dt)       # the row bars are evaluated at the reference g
    rt, bars = _row_bars(x, g_T, muT, dt, dg=dg + eps / 2 * np.abs(ref["g"].astype(np.float64)))
    rr, rb = float(ref["rr"]), float(ref["rb"])
    bars["rr"] = C * (np.sum(2 * r64 * dr + dr * dr) + (CSUM + 1) * EPS64 * rr)
    bars["rb"] = C * (np.sum(b64 * dr) + (CSUM + 1) * EPS64 * np.sum(r64 * b64))
    gmax, s, sx = float(ref["gmax"]), float(ref["scale"]), float(ref["sum_xnorm"])
    dgm = bars["gmax"] / C
    ds = min(1.0, muT / max(gmax - dgm, TINY)) - min(1.0, muT / (gmax + dgm)) if gmax > 0 else 0.0
    host = 4 * EPS64 * (0.5 * (1 + s * s) * rr + abs(s * rb) + muT * sx)
    bars["gap"] = C * (0.5 * (1 + s * s) * bars["rr"] / C + s * bars["rb"] / C + muT * bars["sum_xnorm"] / C
                       + abs(s * rr + rb) * ds + host)
    return ref, bars


def _check_certificate(x, A, b, mu, dt, where):
    import glx
    from glx.certificate import record
    muT = float(dt(mu))
    ref, bars = _cert_bars(x, A, b, mu, dt)
    rec = record(x, A, b, muT)
    got = {"rr": rec[0], "rb": rec[1], "sum_xnorm": rec[2], "gmax": rec[3], "kkt_max": rec[4], "kkt_sq": rec[5]}
    c = glx.certificate(x, A, b, muT)
    got["gap"] = c["gap"]
    worst = {}
    for key, val in got.items():
        err = abs(float(val) - float(ref[key]))
        ratio = err / max(float(bars[key]), TINY)
        print("%s %s: got %.17g ref %.17g err %.3e bar %.3e" % (where, key, float(val), float(ref[key]), err,
                                                               float(bars[key])))
        _note("test 3 %s %s" % (key, _tag(dt)), ratio)
        worst[key] = ratio
    assert all(v <= 1 for v in worst.values()), worst
    assert c["nonzero_rows"] == ref["nonzero_rows"] == int(rec[6])
    assert c["primal"] == 0.5 * rec[0] + muT * rec[2]
    assert c["gap"] >= -bars["gap"]
    return c, ref, bars


def test_certificate_at_the_stored_minimiser():
    _torch()
    with np.load(os.path.join(GOLDEN, "default_xstar.npz")) as z:
        xs, mu, seed = z["x"], float(z["mu"]), int(z["seed"])
    A, b, _, _ = cref.instance(seed, 256, 512, 2, mu)
    c, ref, _ = _check_certificate(xs, A, b, mu, np.float64, "x*")
    print("x*: gap %.3e, gap / primal %.3e, kkt_max %.3e" % (c["gap"], c["rel_gap"], c["kkt_max"]))
    assert c["gap"] <= 1e-9 * c["primal"]


@pytest.mark.parametrize("shape", [(256, 512, 2), (128, 256, 32)], ids=["256x512x2", "128x256x32"])
def test_zero_at_mu_max(shape):
    _torch()
    import glx
    m, n, l = shape
    A, b, _, _ = cref.instance(97006855, m, n, l)
    mm = glx.mu_max(A, b)
    W = np.longdouble
    want = float(cref.mu_max(A.astype(W), b.astype(W)))
    _, bars = _cert_bars(np.zeros((n, l)), A, b, want, np.float64, zero_x=True)
    _note("test 3 mu_max f64", abs(mm - want) / bars["gmax"])
    assert abs(mm - want) <= bars["gmax"]
    c, _, bars = _check_certificate(np.zeros((n, l)), A, b, mm, np.float64, "mu_max")
    assert c["scale"] == 1.0 and c["kkt_max"] == 0.0 and c["nonzero_rows"] == 0
    assert abs(c["gap"]) <= bars["gap"]


def _alm_cases():
    with open(os.path.join(GOLDEN, "alm_dual_index.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", sorted(_alm_cases()))
def test_certificate_at_alm_results(name):
    _torch()
    meta = _alm_cases()[name]
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        x, b = z["x"], z["b"]
    A, _, _, mu = cref.instance(meta["seed"], meta["m"], meta["n"], meta["l"], meta["mu"])
    c, _, _ = _check_certificate(x, A, b, mu, np.float64, name)
    print("%s: gap / primal %.3e, kkt_max %.3e" % (name, c["rel_gap"], c["kkt_max"]))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(100, 130, 3), (96, 192, 64)], ids=["100x130x3", "96x192x64"])
def test_certificate_at_a_random_point(shape, dt):
    _torch()
    m, n, l = shape
    A, b, x0, mu = cref.instance(97006855, m, n, l)
    rng = np.random.default_rng(m * n)
    x = (x0 * (rng.random((n, 1)) < 0.5)).astype(dt)
    _check_certificate(x, A.astype(dt), b.astype(dt), mu, dt, "random %dx%dx%d" % shape)


# ---- 4. interface ----
def test_interface():
    torch = _torch()
    import glx
    A, b, x0, mu = cref.instance(97006855, 64, 128, 16)
    x = x0 * (np.arange(128)[:, None] % 2)
    keep = [a.copy() for a in (x, A, b)]
    c = glx.certificate(x, A, b, mu, row_norms=True)
    assert set(c) == {"primal", "dual", "gap", "rel_gap", "scale", "gmax", "kkt_max", "kkt_fro",
                      "nonzero_rows", "fused", "plan", "row_norms"}
    assert isinstance(c["row_norms"], np.ndarray) and c["row_norms"].shape == (128,)
    assert c["row_norms"].dtype == np.float64 and c["gmax"] == c["row_norms"].max()
    assert c["nonzero_rows"] == 64 and c["gap"] >= 0 and 0 < c["scale"] <= 1
    assert c["rel_gap"] == c["gap"] / abs(c["primal"])
    for a, k in zip((x, A, b), keep):
        assert np.array_equal(a, k)
    assert "row_norms" not in glx.certificate(x, A, b, mu)
    again = glx.certificate(x, A, b, mu, row_norms=True)
    assert np.array_equal(again.pop("row_norms"), c["row_norms"])
    assert again == {k: v for k, v in c.items() if k != "row_norms"}
    xt, At, bt = (torch.from_numpy(a).cuda() for a in (x, A, b))
    kt = [t.clone() for t in (xt, At, bt)]
    ct = glx.certificate(xt, At, bt, mu, row_norms=True)
    assert isinstance(ct["row_norms"], torch.Tensor) and ct["row_norms"].shape == (128,)
    assert np.array_equal(ct.pop("row_norms").cpu().numpy(), c["row_norms"])
    assert ct == {k: v for k, v in c.items() if k != "row_norms"}
    for t, k in zip((xt, At, bt), kt):
        assert torch.equal(t, k)
    assert glx.mu_max(At, bt) == glx.mu_max(A, b) > 0
    with pytest.raises(ValueError):
        glx.certificate(x, A, b, -1.0)
    with pytest.raises(ValueError):
        glx.certificate(x[:-1], A, b, mu)
    with pytest.raises(glx.GlxError):
        glx.certificate(x, A, b, mu, fused=3)
    c32 = glx.certificate(x.astype(np.float32), A.astype(np.float32), b.astype(np.float32), mu)
    assert abs(c32["primal"] - c["primal"]) <= 1e-4 * c["primal"]


# ---- 5. driver ----
def _table(text):
    lines = [ln for ln in text.splitlines() if ln.startswith("|")]
    return [[c.strip() for c in ln.strip("|").split("|")] for ln in lines]


def test_driver_certify_columns(tmp_path, capsys):
    _torch()
    from glx import driver
    names = ["ProxGD Primal", "FProxGD Primal"]
    argv = ["--log", str(tmp_path / "opt.log"), "--dest_dir", str(tmp_path / "fig"), "--solvers", ",".join(names)]
    assert driver.main(argv + ["--certify"]) == 0
    with_flag = _table(capsys.readouterr().out)
    assert with_flag[0] == ["solver", "cpu", "iter", "optval", "sparsity", "err-to-exact", "err-to-x*", "gap", "kkt"]
    buf = io.StringIO()
    plain = driver.run({k: v for k, v in driver._glx_solvers().items() if k in names}, stream=buf)
    without = _table(buf.getvalue())
    assert without[0] == with_flag[0][:-2]
    for a, b_ in zip(with_flag[2:], without[2:]):      # the same run: everything but the stopwatch
        assert a[0] == b_[0] and a[2:7] == b_[2:]
    assert [r[0] for r in with_flag[2:]] == names
    _, _, _, mu, A, b, *_ = driver.gen_data()
    for row in with_flag[2:]:
        assert re.fullmatch(r"\d\.\d\dE[+-]\d\d", row[7].lstrip("-")) and re.fullmatch(r"\d\.\d\dE[+-]\d\d", row[8])
        _, bars = _cert_bars(plain["xs"][row[0]], A, b, mu, np.float64)
        assert float(row[7]) >= -bars["gap"]
        assert float(row[8]) >= 0
    log = open(tmp_path / "opt.log").read()
    assert log.count("gap: ") == 2 and log.count("kkt: ") == 2
