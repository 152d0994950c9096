"""The dual ALM solver on the GPU: its inner step one launch at a time, its inner loop, whole solves.

Reached through glx_alm_inner_step, glx_alm_inner_run (glx.kernels) and glx_alm_dual_solve
(glx.alm, gl_ALM_dual.gl_Alm_dual). References: the formulas of gl_ALM_dual.py:45-47, 56-61 written
below in np.longdouble (nothing imported from glx), tests/alm_dual_ref.py (the restructured
iteration in NumPy float64) and the reference solver's recorded runs (tests/golden/alm_dual_*.npz,
made by tests/golden/make_alm_dual_golden.py). float64 only, as the solver.

1. One inner step. Scalars reach the kernel as doubles (t, mu, gamma, a1 = 1 - gamma+ formed in
double, g+ = gamma+); eps = 2^-52 (u = eps / 2 the unit roundoff). Per element j of a row, with
a_j = |y_j| + t (|P_j| + |J_j|) >= |w_j| and N = ||a||_2. Term by term, to first order:
  P    form 0: the S slabs are added in slab order, S - 1 roundings: dP_j <= (S - 1) eps / 2 sum_s |P_s,j|
       (0 for one slab); form 1: P = Qn^T y on MFMA, a dot product of n terms:
       dP_j <= (n + 2) eps sum_k |Qn_kj| |y_k|  (the bar of test_gpu_admm.py for A^T Z).
  w    q = P + J rounds once, t q once, y - t q once, each at most u a_j:
         dw_j <= t dP_j + 3 / 2 eps a_j.
  nrm  the l squares (u each), <= 5 additions (1 in a lane, 4 shuffle levels) and the root: relative
       <= (l / 2 + 2) eps on the computed w, plus ||dw||_2 from w itself:
         dn <= (l / 2 + 2) eps N + ||dw||_2.
  d    max(nrm, mu) is 1-Lipschitz in nrm: dd <= dn on either side of the switch and across it.
  u+   (mu w) / d: two roundings (eps |u+|), dw scaled by mu / d <= 1, dd relative to d:
         du_j <= dw_j + |u+_j| (eps + dn / d).
  v+   u+ - u rounds once, the division once, the sum once:
         dv_j <= du_j / gamma + eps |u+_j - u_j| / gamma + eps / 2 |v+_j|.
  y+   a1 u+ and g+ v+ round once each, their sum once:
         dy_j <= |a1| du_j + g+ dv_j + eps / 2 (|a1 u+_j| + |g+ v+_j| + |y+_j|).
Each bar is doubled (C = 2, the only slack) for the second-order terms dropped above. The inputs
hold rows outside the ball, rows strictly inside it, an all-zero row (which stays zero), a row with
||w|| within a few ulp of mu and, in a second run, one NaN row: that row comes out NaN and every
other row is bit-identical to the first run. gamma_next = 0 leaves a NaN-filled y_out untouched.
A row of l values is held by LPR lanes with EPL values each. The generic shapes' l select
(LPR, EPL) = 1 (1, 1), 2 (2, 1), 3 (4, 1), 8 (8, 1), 17 and 32 (16, 2) of k_alm_inner, and the fused
shapes run the panel layout at l = 16 and 32; with (16, 1) of the several-trip cases that is every
instantiation. All of those are one trip of a dozen workgroups at most. test_inner_step_several_trips
runs form 0 at (l, n) = (1, 131077), (2, 65541), (3, 32771), (8, 16389), (16, 8200), (17, 8200),
(32, 8200), on one slab and on three: each 5 to 8 rows past the 512 * 256 / LPR rows the capped grid
of 512 workgroups takes in one trip, so two trips, the second ragged; u+ and y+ of the rows on both
sides of the boundary are bit-identical to those of a launch of their own. The step has no sums,
so its bars do not depend on the trips.

2. The fused form (form 1, k_atr_alm) against form 0 (k_alm_inner_panel) on the product that
kernels.gradient(Qn, y) wrote: every bit of u+ and y+, at the shapes whose plan fuses, and on every
tile built for a fused epilogue by name (GLX_ATR_VARIANT, with one and two K splits where the tile
takes splits; the tile and S are asserted from the describe string) at n = 128, l = 16 and n = 192,
l = 32. Both forms are also held to test 1's bars there (P's bar is form 1's).

3. The inner loop (glx_alm_inner_run) against the NumPy loop: within 1e-10 of max |u|. The step
y -> u+ is non-expansive for t rho <= 1 (a projection after a gradient step of step t <= 1 / ||Qn||),
and the extrapolation weights are bounded, so the per-step rounding (about l eps relative) adds at
most linearly over 500 steps: 500 * 34 * 2.2e-16 = 3.8e-12, under 1e-10 with room for the product's
own n-term dot products. fused = 1 and fused = 2 give the same bits, and so does a second run.

4.-6. Whole solves: see each test.

Measured on an MI355X, worst error / bound over all cases (the module prints this table when its
tests are over, pytest -s):
  test 1   u+ 0.161 (generic) 0.121 (panel) 0.028 (fused)   y+ 0.174 0.138 0.138
           rows at the switch: 1 per case (the constructed one)
  test 3   inner loop 6.9e-6 of its bar (6.9e-16 of max |u|, 500 steps included)
  test 4   k identical to the reference's in all 7 fixtures, with fused = 0 and fused = 2; f_hist
           within 3.7e-11 relative (the m > n case; the others <= 7.4e-14); x within 9.0e-13 of
           max |x|
None is above 1.
"""
import json
import logging
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from tile_cases import ROWS as TILE_ROWS

import alm_dual_ref

pytestmark = pytest.mark.gpu

T_STEP, MU = 1e-2, 1e-2
C = 2.0
EPS = float(np.finfo(np.float64).eps)
W = np.longdouble
MEASURED = {}


def _note(key, ratio):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nworst error / bound:", json.dumps({k: float("%.3g" % v) for k, v in sorted(MEASURED.items())}))


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


FUSED_SHAPES = [(128, 16), (128, 32), (192, 32)]
# l -> (LPR, EPL) of launch_alm_inner: 1 (1, 1), 2 (2, 1), 3 (4, 1), 8 (8, 1), 17 and 32 (16, 2); the
# fused shapes run the panel layout (LPR 16; EPL 1 at l = 16, 2 at l = 32)
GENERIC_SHAPES = [(130, 3), (128, 1), (67, 32), (130, 2), (130, 8), (131, 17)]


def _step_inputs(n, l, S, seed):
    """P (S slabs), y, J, u of n x l: row kinds by index (0 outside the ball, 1 inside, 2 all-zero,
    3 at the switch, then random in / out)."""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n, l))
    J = rng.standard_normal((n, l)) * 0.5
    u = rng.standard_normal((n, l)) * MU / math.sqrt(l)
    w = rng.standard_normal((n, l)) * 0.05                         # ||w|| ~ 0.05 sqrt(l): outside (l > 1)
    inside = rng.random(n) < 0.4
    inside[:4] = [False, True, False, False]
    w[0] = 5 * MU * np.sign(w[0] + (w[0] == 0))                   # outside for every l
    for i in np.nonzero(inside)[0]:
        w[i] *= 0.3 * MU / np.linalg.norm(w[i])
    y = w + T_STEP * (P + J)
    P[2] = J[2] = u[2] = y[2] = 0
    ws = rng.standard_normal(l)
    P[3] = J[3] = 0
    y[3] = ws * (MU * (1 + 2 * EPS) / np.linalg.norm(ws))
    if S > 1:   # slabs that add up to about P, with cancellation between them
        parts = rng.standard_normal((S - 1, n, l))
        parts[:, 2] = 0
        parts[:, 3] = 0
        P = np.concatenate([parts, (P - parts.sum(axis=0))[None]], axis=0)
    else:
        P = P[None]
    return P, y, J, u


def _step_inputs_large(n, l, S, seed):
    """_step_inputs for the several-trip cases, drawn in whole arrays (the same row kinds)."""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n, l))
    J = rng.standard_normal((n, l)) * 0.5
    u = rng.standard_normal((n, l)) * MU / math.sqrt(l)
    w = rng.standard_normal((n, l)) * 0.05
    inside = rng.random(n) < 0.4
    inside[:4] = [False, True, False, False]
    w[0] = 5 * MU * np.sign(w[0] + (w[0] == 0))
    w = np.where(inside[:, None], w * (0.3 * MU / np.linalg.norm(w, axis=1, keepdims=True)), w)
    y = w + T_STEP * (P + J)
    P[2] = J[2] = u[2] = y[2] = 0
    ws = rng.standard_normal(l)
    P[3] = J[3] = 0
    y[3] = ws * (MU * (1 + 2 * EPS) / np.linalg.norm(ws))
    if S > 1:
        parts = rng.standard_normal((S - 1, n, l))
        parts[:, 2] = 0
        parts[:, 3] = 0
        P = np.concatenate([parts, (P - parts.sum(axis=0))[None]], axis=0)
    else:
        P = P[None]
    return P, y, J, u


def _step_reference(Pw, dP, y, J, u, gamma, gnext):
    """The step in longdouble from the float64 inputs and scalars, and the bars. Pw: the exact P."""
    l = y.shape[1]
    t, mu, g, a1, gn = W(T_STEP), W(MU), W(gamma), W(np.float64(1.0 - gnext)), W(gnext)
    yw, Jw, uw = y.astype(W), J.astype(W), u.astype(W)
    w = yw - t * (Pw + Jw)
    nrm = np.sqrt(np.sum(w * w, axis=1, keepdims=True))
    d = np.maximum(nrm, mu)
    un = mu * w / d
    vn = uw + (un - uw) / g
    yn = a1 * un + gn * vn
    a = np.abs(yw) + t * (np.abs(Pw) + np.abs(Jw))
    N = np.sqrt(np.sum(a * a, axis=1, keepdims=True))
    dw = t * dP + 1.5 * EPS * a
    dn = (l / 2 + 2) * EPS * N + np.sqrt(np.sum(dw * dw, axis=1, keepdims=True))
    du = dw + np.abs(un) * (EPS + dn / d)
    dv = du / g + EPS * np.abs(un - uw) / g + EPS / 2 * np.abs(vn)
    dy = np.abs(a1) * du + gn * dv + EPS / 2 * (np.abs(a1 * un) + np.abs(gn * vn) + np.abs(yn))
    return {"u": un, "y": yn, "bu": C * du, "by": C * dy, "amb": int(np.sum(np.abs(nrm - mu) <= dn))}


def _check_step(got_u, got_y, ref, tag):
    tiny = np.finfo(np.float64).tiny
    for key, got, bar in (("u", got_u, ref["bu"]), ("y", got_y, ref["by"])):
        err = np.abs(got.astype(W) - ref[key])
        ratio = float(np.max(err / np.maximum(bar, tiny)))
        _note(key + "+ " + tag, ratio)
        assert np.all(err <= bar), (key, ratio)
    assert not got_u[2].any() and not got_y[2].any()     # the all-zero row stays zero
    assert 1 <= ref["amb"] <= 4
    _note("rows at the switch", ref["amb"])


def _run_step(form, Pd, yd, Jd, ud, gamma, gnext, Qnd=None):
    from glx import kernels
    if form == 1:
        return kernels.alm_inner_step(yd, ud, Jd, gamma, gnext, T_STEP, MU, Qn=Qnd, form=1)
    return kernels.alm_inner_step(yd, ud, Jd, gamma, gnext, T_STEP, MU, P=Pd, form=0)


def _step_case(form, P, y, J, u, Pw, dP, gamma, gnext, fuses, Qn=None):
    """One launch against the longdouble step on the exact product Pw with its bar dP, then
    gamma_next = 0 and the NaN row; returns the first run's u+, y+."""
    torch = _torch()
    n, l = y.shape
    ref = _step_reference(Pw, dP, y, J, u, gamma, gnext)
    Pd, yd, Jd, ud = _dev(P), _dev(y), _dev(J), _dev(u)
    Qnd = _dev(Qn) if Qn is not None else None
    out = _run_step(form, Pd, yd, Jd, ud, gamma, gnext, Qnd)
    gu, gy = out["u"].cpu().numpy(), out["y"].cpu().numpy()
    _check_step(gu, gy, ref, "panel" if fuses and form == 0 else ("fused" if form == 1 else "generic"))
    # gamma_next = 0: the same u+, and a NaN-filled y_out is left as it was
    last = _run_step(form, Pd, yd, Jd, ud, gamma, 0.0, Qnd)
    assert np.array_equal(last["u"].cpu().numpy(), gu)
    assert torch.isnan(last["y"]).all()
    # one NaN in the last row (in J, which is row-local in every arm; a NaN in y would reach every
    # row of Qn^T y): that row NaN, every other row bit-identical
    J2 = J.copy()
    J2[n - 1, l // 2] = np.nan
    out2 = _run_step(form, Pd, yd, _dev(J2), ud, gamma, gnext, Qnd)
    for key, first in (("u", gu), ("y", gy)):
        v = out2[key].cpu().numpy()
        assert np.isnan(v[n - 1]).all(), key
        assert np.array_equal(v[:n - 1], first[:n - 1]), key
    return gu, gy


@pytest.mark.parametrize("gamma,gnext", [(1.0, 2 / 3), (2 / 8, 2 / 9)], ids=["first", "i7"])
@pytest.mark.parametrize("arm", ["S1", "S3", "fused"])
@pytest.mark.parametrize("n,l", FUSED_SHAPES + GENERIC_SHAPES)
def test_inner_step_against_longdouble(n, l, arm, gamma, gnext):
    torch = _torch()
    from glx import _lib
    fuses = "inner step=fused" in _lib.alm_describe(_lib.GLX_F64, n, n, l)
    assert fuses == ((n, l) in FUSED_SHAPES)
    if arm == "fused" and not fuses:
        # the generic shapes have no third arm; their form 1 is refused instead
        z = torch.zeros((n, l), dtype=torch.float64, device="cuda")
        Q = torch.zeros((n, n), dtype=torch.float64, device="cuda")
        with pytest.raises(_lib.GlxError) as e:
            _run_step(1, None, z, z, z, gamma, gnext, Qnd=Q)
        assert e.value.code == 1   # GLX_E_INVALID
        return
    S = 3 if arm == "S3" else 1
    P, y, J, u = _step_inputs(n, l, S, seed=1000 * n + l)
    Qn = None
    if arm == "fused":   # P = Qn^T y with a Qn that is not symmetric (the kernel transposes)
        rng = np.random.default_rng(n + l)
        Qn = rng.standard_normal((n, n)) / math.sqrt(n)
        Qn[:, 2] = 0       # P[2] = 0 for the all-zero row and P[3] = 0 for the row at the switch
        Qn[:, 3] = 0
        # y so that w keeps the drawn row kinds under this P: the fixed point of
        # y = w + t (Qn^T y + J), a contraction (t ||Qn|| ~ 0.02); rows 2 and 3 stay as drawn
        w = y - T_STEP * (P[0] + J)
        for _ in range(20):
            y = w + T_STEP * (Qn.T @ y + J)
        assert not y[2].any()
        Pw = Qn.astype(W).T @ y.astype(W)
        dP = (n + 2) * EPS * (np.abs(Qn).astype(W).T @ np.abs(y).astype(W))
    else:
        Pw = P.astype(W).sum(axis=0)
        dP = (S - 1) * EPS / 2 * np.abs(P).astype(W).sum(axis=0)
    _step_case(1 if arm == "fused" else 0, P, y, J, u, Pw, dP, gamma, gnext, fuses, Qn)


# one n past a single trip of the 512-workgroup grid (512 * 256 / LPR rows) per layout: LPR 1, 2, 4,
# 8, then LPR 16 with EPL 1, a ragged EPL 2 and a full EPL 2; two trips each, the second of 5 to 8 rows
SEVERAL_TRIPS = [(1, 131077), (2, 65541), (3, 32771), (8, 16389), (16, 8200), (17, 8200), (32, 8200)]


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("l,n", SEVERAL_TRIPS)
def test_inner_step_several_trips(l, n, S):
    """Test 1's form 0 past one trip, on the generic layout (the plan of (n, n, l) does not fuse,
    asserted from the describe string). The step has no sums, so the bars are test 1's as they stand.
    Then the rows on both sides of the trip boundary run again as an input of their own, in one
    trip: u+ and y+ of a row depend on neither n nor the trip, so they come back bit for bit (the
    wrapper pre-fills them with NaN)."""
    from glx import _lib
    assert "inner step=fused" not in _lib.alm_describe(_lib.GLX_F64, n, n, l)
    lpr = 1
    while lpr < min(l, 16):
        lpr *= 2
    per_trip = 512 * 256 // lpr
    assert -(-n // per_trip) == 2 and 0 < n - per_trip < 256 // lpr
    gamma, gnext = ((1.0, 2 / 3), (2 / 8, 2 / 9))[(l + S) % 2]
    P, y, J, u = _step_inputs_large(n, l, S, seed=1000 * n + l)
    Pw = P.astype(W).sum(axis=0)
    dP = (S - 1) * EPS / 2 * np.abs(P).astype(W).sum(axis=0)
    gu, gy = _step_case(0, P, y, J, u, Pw, dP, gamma, gnext, False)
    rows = slice(per_trip - 251, n)
    ns = n - (per_trip - 251)
    assert "inner step=fused" not in _lib.alm_describe(_lib.GLX_F64, ns, ns, l)   # the same layout
    part = _run_step(0, _dev(P[:, rows]), _dev(y[rows]), _dev(J[rows]), _dev(u[rows]), gamma, gnext)
    assert np.array_equal(part["u"].cpu().numpy().view(np.uint64), gu[rows].view(np.uint64))
    assert np.array_equal(part["y"].cpu().numpy().view(np.uint64), gy[rows].view(np.uint64))


# the planner's own tile and splits at FUSED_SHAPES, then every fused tile by name (GLX_ATR_VARIANT)
# with the K splits it takes under an epilogue, at NT = 1 and at NT = 2 with n not a power of two:
# four-wave, eight-wave (1028) and 32-column (38, 1038) row ownership, split and not
FUSED_TILES = [(8, (1, 2)), (1008, (1, 2)), (1028, (1, 2)), (38, (1,)), (1038, (1,))]
FUSED_ARMS = [(n, l, None, None) for n, l in FUSED_SHAPES] + \
    [(n, l, tile, S) for n, l in ((128, 16), (192, 32)) for tile, Ss in FUSED_TILES for S in Ss]
ATR_NAMES = {row[1]: row[4] for row in TILE_ROWS if row[0] == "atr"}   # tile -> its name in a describe string


@pytest.mark.parametrize("n,l,tile,S", FUSED_ARMS,
                         ids=["%d-%d" % a[:2] + ("" if a[2] is None else "-t%d-S%d" % a[2:]) for a in FUSED_ARMS])
def test_fused_step_is_bit_identical_to_unfused(n, l, tile, S, monkeypatch):
    torch = _torch()
    from glx import _lib, kernels
    if tile is not None:
        monkeypatch.setenv("GLX_ATR_VARIANT", str(tile))
        monkeypatch.setenv("GLX_ATR_S", str(S))
    d = _lib.alm_describe(_lib.GLX_F64, n, n, l)
    assert "inner step=fused" in d, d
    if tile is not None:   # the named tile and S were planned
        assert d.split("Qn y=")[1].split(";")[0] == ATR_NAMES[tile].format(S=S), d
    rng = np.random.default_rng(7 * n + l)
    A = rng.standard_normal((n // 2, n))
    Qn = alm_dual_ref.inner_matrix(A, alm_dual_ref.inverse_factor(A, 100.0), 100.0)
    _, y, J, u = _step_inputs(n, l, 1, seed=n + l)
    Qnd, yd, Jd, ud = _dev(Qn), _dev(y), _dev(J), _dev(u)
    Pd = kernels.gradient(Qnd, yd)
    Pw = Qn.astype(W).T @ y.astype(W)
    dP = (n + 2) * EPS * (np.abs(Qn).astype(W).T @ np.abs(y).astype(W))
    for gamma, gnext in ((1.0, 2 / 3), (2 / 8, 2 / 9), (2 / 501, 0.0)):
        f1 = _run_step(1, None, yd, Jd, ud, gamma, gnext, Qnd)
        f0 = _run_step(0, Pd, yd, Jd, ud, gamma, gnext)
        assert torch.equal(f1["u"].view(torch.int64), f0["u"].view(torch.int64))
        assert torch.equal(f1["y"].view(torch.int64), f0["y"].view(torch.int64))   # (NaN bits where unwritten)
        # and the step itself under test 1's bars (both forms: they are the same bits)
        ref = _step_reference(Pw, dP, y, J, u, gamma, gnext)
        for key, bar in (("u", "bu"), ("y", "by")) if gnext != 0.0 else (("u", "bu"),):
            err = np.abs(f1[key].cpu().numpy().astype(W) - ref[key])
            _note(key + "+ tiles", float(np.max(err / np.maximum(ref[bar], np.finfo(np.float64).tiny))))
            assert np.all(err <= ref[bar]), key


# ---------------------------------------------------------------------------------------------
# the inner loop
# ---------------------------------------------------------------------------------------------
_LOOP = {}


def _loop_case(n, l):
    """Qn of a random A (m = n / 2, rho = 100, so t rho = 1), J, and the NumPy loop's u per iters."""
    if (n, l) not in _LOOP:
        rng = np.random.default_rng(31 * n + l)
        A = rng.standard_normal((n // 2, n))
        Qn = alm_dual_ref.inner_matrix(A, alm_dual_ref.inverse_factor(A, 100.0), 100.0)
        J = rng.standard_normal((n, l)) * 0.5
        _LOOP[(n, l)] = (Qn, J, {})
    return _LOOP[(n, l)]


@pytest.mark.parametrize("iters", [1, 2, 7, 500])
@pytest.mark.parametrize("n,l", [(128, 16), (130, 3)])
def test_inner_loop_against_numpy(n, l, iters):
    torch = _torch()
    from glx import kernels
    Qn, J, cache = _loop_case(n, l)
    if iters not in cache:
        cache[iters] = alm_dual_ref.inner_loop(Qn, J, iters, T_STEP, MU)
    want = cache[iters]
    Qnd, Jd = _dev(Qn), _dev(J)
    got = {f: kernels.alm_inner_run(Qnd, Jd, iters, T_STEP, MU, fused=f) for f in (0, 1, 2)}
    err = float(np.max(np.abs(got[0].cpu().numpy() - want)) / np.max(np.abs(want)))
    _note("inner loop", err / 1e-10)
    assert err <= 1e-10, err
    assert torch.equal(got[1].view(torch.int64), got[2].view(torch.int64))
    assert torch.equal(got[0].view(torch.int64), got[1].view(torch.int64))
    again = kernels.alm_inner_run(Qnd, Jd, iters, T_STEP, MU, fused=1)
    assert torch.equal(again.view(torch.int64), got[1].view(torch.int64))


def test_inner_loop_bits_with_several_panels():
    """n = 192 (three panels, three K splits): fused = 1, fused = 2 and a repeat give the same bits,
    which a y+ written over the product's operand would break."""
    torch = _torch()
    from glx import kernels
    Qn, J, _ = _loop_case(192, 32)
    Qnd, Jd = _dev(Qn), _dev(J)
    a = kernels.alm_inner_run(Qnd, Jd, 25, T_STEP, MU, fused=1)
    b = kernels.alm_inner_run(Qnd, Jd, 25, T_STEP, MU, fused=2)
    c = kernels.alm_inner_run(Qnd, Jd, 25, T_STEP, MU, fused=1)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.equal(a.view(torch.int64), c.view(torch.int64))
    want = alm_dual_ref.inner_loop(Qn, J, 25, T_STEP, MU)
    assert np.max(np.abs(a.cpu().numpy() - want)) <= 1e-10 * np.max(np.abs(want))


# ---------------------------------------------------------------------------------------------
# whole solves
# ---------------------------------------------------------------------------------------------
with open(os.path.join(GOLDEN, "alm_dual_index.json")) as _fh:
    INDEX = json.load(_fh)
CASES = sorted(INDEX)


def _case(name):
    from test_alm_dual_cpu import load_case
    return load_case(name)


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(np.asarray(want))))


@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("name", CASES)
def test_solve_against_reference(name, fused):
    """k identical; fval, f_hist, f_hist_best within 1e-8 relative (the project's fp64 parity bar);
    x within 1e-6 of max |x|; the counters as specified."""
    _torch()
    from gl_ALM_dual import gl_Alm_dual
    meta, arrs, A, b, x0, mu = _case(name)
    x, k, out = gl_Alm_dual(x0, A, b, mu, {**meta["opts"], "fused": fused})
    fh, fb = np.asarray(out["f_hist"]), np.asarray(out["f_hist_best"])
    xe = float(np.max(np.abs(x - arrs["x"])) / np.max(np.abs(arrs["x"])))
    print(name, "fused", fused, "k", k, "ref k", int(arrs["k"]), "fval rel", _rel(out["fval"], arrs["fval"]),
          "f_hist rel", _rel(fh[:len(arrs["f_hist"])], arrs["f_hist"][:len(fh)]), "x", xe)
    assert k == int(arrs["k"])
    assert len(fh) == k and len(fb) == k
    _note("f_hist", _rel(fh, arrs["f_hist"]) / 1e-8)
    _note("x", xe / 1e-6)
    assert _rel(out["fval"], arrs["fval"]) <= 1e-8
    assert _rel(fh, arrs["f_hist"]) <= 1e-8
    assert _rel(fb, arrs["f_hist_best"]) <= 1e-8
    assert xe <= 1e-6
    g = out["glx"]
    assert g["ax_calls"] == 2 * k + 1 and g["atr_calls"] == 2 * k and g["syncs"] == k
    assert g["k_calls"] == 2 * k and g["inner_steps"] == 500 * k
    assert g["fused"] == (fused != 2 and "inner step=fused" in g["plan"])
    assert g["fused"] == (fused != 2 and meta["l"] in (16, 32) and meta["n"] % 64 == 0)
    assert out["tt"] >= g["setup_s"] > 0


OPTION_CASES = [{"maxit": 5}, {"converge_len": 3}, {"tau": 1.0}, {"thres": 1e-2}, {"inner_iters": 50},
                {"max_total_iters": 4}, {"maxit": 0}]


@pytest.mark.parametrize("opts", OPTION_CASES, ids=lambda o: "_".join("%s%g" % kv for kv in o.items()))
def test_options_against_restatement(opts):
    _torch()
    from glx import alm
    meta, arrs, A, b, x0, mu = _case("alm_dual_64x128x16")
    given = dict(opts)
    x, k, out = alm.solve(x0, A, b, mu, given)
    assert given == opts                                  # the caller's dict is not mutated
    xr, kr, outr = alm_dual_ref.gl_alm_dual(x0, A, b, mu, dict(opts))
    assert k == kr
    assert len(out["f_hist"]) == k
    if k:
        assert _rel(out["f_hist"], outr["f_hist"]) <= 1e-8
        assert _rel(out["f_hist_best"], outr["f_hist_best"]) <= 1e-8
    else:
        assert np.array_equal(x, x0) and out["f_hist"] == []
    assert _rel(out["fval"], outr["fval"]) <= 1e-8
    assert np.max(np.abs(x - xr)) <= 1e-6 * np.max(np.abs(xr))
    inner = opts.get("inner_iters", 500)
    g = out["glx"]
    assert (g["ax_calls"], g["atr_calls"], g["syncs"], g["k_calls"], g["inner_steps"]) == \
        (2 * k + 1, 2 * k, k, 2 * k, inner * k)


def test_drop_in_module_contract(caplog):
    """NumPy in, NumPy out; torch in, torch out; x0 untouched; the debug line replayed."""
    torch = _torch()
    from gl_ALM_dual import gl_Alm_dual
    meta, arrs, A, b, x0, mu = _case("alm_dual_256x512x2")
    x0_before = x0.copy()
    opts = {"maxit": 4, "not_an_option": 1}
    opts_before = dict(opts)
    with caplog.at_level(logging.DEBUG, logger="opt"):
        x, k, out = gl_Alm_dual(x0, A, b, mu, opts)
    assert isinstance(x, np.ndarray) and x.dtype == np.float64 and x.shape == x0.shape
    assert isinstance(k, int) and k == 4
    assert np.array_equal(x0, x0_before) and opts == opts_before
    assert {"tt", "fval", "f_hist", "f_hist_best", "glx"} <= set(out)
    assert np.allclose(out["f_hist"], arrs["f_hist"][:4], rtol=1e-8, atol=0)
    assert not out["glx"]["fused"]                        # l = 2: the generic arm, two launches a step
    lines = [r.getMessage() for r in caplog.records if r.name == "opt"]
    assert len(lines) == 4
    sp = float(np.sum(np.abs(x) > 1e-6 * np.max(np.abs(x))) / x.size)
    assert lines[0].startswith("iter=     1, objective= ")
    assert lines[-1] == "iter= {:5}, objective= {:10E}, sparsity= {:3f}".format(4, float(out["f_hist"][-1]), sp)
    xt, kt, outt = gl_Alm_dual(torch.from_numpy(x0).cuda(), torch.from_numpy(A).cuda(),
                               torch.from_numpy(b).cuda(), mu, opts)
    assert isinstance(xt, torch.Tensor) and xt.is_cuda and kt == 4
    assert np.array_equal(xt.cpu().numpy(), x)
