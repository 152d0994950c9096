"""The primal ADMM solver on the GPU: its row kernel one launch at a time, then whole solves.

Reached through glx_admm_primal_step (glx.kernels) and glx_admm_primal_solve (glx.admm_primal,
gl_ADMM_primal.gl_Admm_primal). References: the formulas of gl_ADMM_primal.py:47-51, 78-84 written
below in NumPy in the next wider type (np.longdouble for f64 inputs, np.float64 for f32 inputs;
nothing imported from glx), the reference solver's recorded runs (tests/golden/admm_primal_*.npz,
made by tests/golden/make_admm_primal_golden.py) for whole solves, and tests/admm_primal_ref.py
where options vary.

1. The row kernel, both forms, S = 1 and S = 3 slabs. Scalars are rounded to T first, as the
launcher does: rho, er = eta rho, em = eta mu, tr = tau rho (formed in double, then rounded) and
thres. eps = T's machine epsilon, u = eps / 2 the unit roundoff. Term by term, first order:
  P    the S slabs are added in slab order, S - 1 roundings: dP_j <= (S - 1) u sum_s |slab_sj|.
  y+   direct: y+ = P, dy_j = dP_j. Woodbury: (w - P) / rho, the difference and the quotient round
       once each, relative to the result: dy_j <= dP_j / rho + eps |y+_j|.
  p    t1 = x - y+ (dy + u |t1|), t2 = z / rho (u |t2|), t3 = t1 - t2 (+ u |t3|), t4 = er t3
       (+ u |t4|, |t4| = er |t3|), p = x - t4 (+ u |p|):
         dp_j <= er dy_j + u (er (|t1| + |t2| + 2 |t3|) + |p_j|).
  nr   the l squares (u each), <= 6 additions (2 in a lane, 4 shuffle levels) and the root:
       relative <= (l / 2 + 2) eps on the computed p, plus ||dp||_2 from p itself:
         dn <= (l / 2 + 2) eps nr + ||dp||_2.
  c    max(nr - em, 0): the difference rounds once and max(., 0) is 1-Lipschitz, so
         dc <= dn + u c
       on either side of the switch and across it: a row whose norm sits within dn of em needs no
       looser bar than its neighbours. Such rows are still counted: at most 4 per case.
  d    (nr < thres) + nr: the indicator is a jump in the reference itself, so the inputs hold no
       row within dn of thres (asserted before the GPU is looked at); then d = nr exactly where
       nr >= thres and 1 + nr rounds once below it: dd <= dn + [nr < thres] u d.
  x+   (p c) / d: the product and the quotient round once each:
         dx_j <= (c dp_j + |p_j| dc) / d + |x+_j| (eps + dd / d).
  r    x+ - y+ rounds once:              dr_j <= dx_j + dy_j + u |r_j|.
  z+   z - tr r, two roundings:          dz_j <= tr dr_j + u (tr |r_j| + |z+_j|).
  s    y+ - y rounds once:               ds_j <= dy_j + u |s_j|.
  w+   a1 = ATb - z+, a2 = rho x+, a1 + a2: dw_j <= dz_j + rho dx_j + u (|a1| + |a2| + |w+_j|).
  sum_i ||x+_i||  per row ||dx_i||_2 + (l / 2 + 2) eps ||x+_i|| (as nr), + CSUM eps64 sum |term|
       for the fp64 accumulation (CSUM = 32 additions deep: a few per thread, 8 levels in the
       workgroup, 12 over the workgroup partials). A thread adds one more row norm in every further
       trip of its workgroup: the several-trip cases take CSUM + trips - 1 (33 at their two trips).
  max |x+|        max_j dx_j (max is 1-Lipschitz in every element).
Each bar is doubled (C = 2) for the second-order terms dropped above. Two parameter sets: the
defaults (eta = 100: er = 1, em = 1) and eta = 1e-2 (em = 1e-4 < thres): only the second lets a row
with 1e-4 < ||p|| < 1e-3 come out non-zero through the 1 + nr denominator. The inputs hold, where n
allows, rows above the threshold em, rows below it (exact zeros), an all-zero row, a row with ||p||
within a few ulp of em, one row in the nr < thres regime and, in a second run, one NaN row: that
row comes out NaN, every other row bit-identical to the first run, both sums NaN.
A row of l values is held by LPR lanes with EPL values each; the l of test 1 select (LPR, EPL) =
1 (1, 1), 2 (2, 1), 3 (4, 1), 5 and 8 (8, 1), 16 (16, 1), 17 and 32 (16, 2): every instantiation of
k_admm_primal, with a ragged row at LPR 4, LPR 8 and EPL 2, each in one trip of at most 17
workgroups. test_row_kernel_several_trips runs (l, n) = (1, 131077), (2, 65541), (3, 32771),
(8, 16389), (16, 8200), (17, 8200), (32, 8200), the direct form on one slab with the defaults and the
Woodbury form on three slabs with eta = 1e-2: each 5 to 8 rows past the 512 * 256 / LPR rows the
capped grid of 512 workgroups takes in one trip, so two trips, the second ragged; the six outputs of
the rows on both sides of the boundary are bit-identical to those of a launch of their own.

2. Slab order: S = 3 slabs give the bits of the same product summed in slab order beforehand.

3.-6. Whole solves: see each test.

Measured on an MI355X, worst error / bound over all cases (f64, f32); the module prints this table
when its tests are over (pytest -s):
  test 1   x+ 0.288 0.301   y+ 0.395 0.388   z+ 0.444 0.462   r 0.469 0.484   s 0.500 0.500
           w+ 0.462 0.463   sum ||x+_i|| 0.013 0.033   max |x+| 0.055 0.051
           rows at the switch: the constructed one per case with n > 3, and one more in two of the
           several-trip cases in f32; rows at thres: 0
           (s is one rounding of an exact difference where S = 1, bar 2 u |s|: 0.5 is its ceiling)
  test 3   k identical in all 22 solves; f_hist within 1.5e-9 relative (direct) and 1.9e-9
           (Woodbury), both at (96, 192, 1); x within 8.6e-11 / 1.7e-10 of max |x|
  test 4   fp32 (192, 128, 16): k identical, fval within 1.2e-7 relative
  test 5   f_hist against tests/admm_primal_ref.py within 1.1e-10 relative over the seven option sets
None is above 1.
"""
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RHO, TAU, MU, THRES = 1e-2, (1 + math.sqrt(5)) * 0.5, 1e-2, 1e-3
ETAS = {"default": 100.0, "small_eta": 1e-2}
C = 2.0
CSUM = 32
OUTS = ("x", "y", "z", "r", "s", "w")
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


def _unit(rng, l):
    v = rng.standard_normal(l)
    return v / np.linalg.norm(v)


def _row_inputs(n, l, dt, form, S, eta, seed):
    """slabs (S, n, l), x, y, z, w, ATb of n x l in dt. Row kinds by index: 0 above the threshold,
    1 below it, 2 all-zero, 3 at the switch ||p|| = em, 4 in the nr < thres regime, then random
    above / below. Rows are built in float64 from the p they should give, then rounded to dt."""
    rng = np.random.default_rng(seed)
    er, em = eta * RHO, eta * MU
    x = rng.standard_normal((n, l))
    y = rng.standard_normal((n, l))
    z = rng.standard_normal((n, l)) * 1e-2
    w = rng.standard_normal((n, l))
    atb = rng.standard_normal((n, l))
    yn = rng.standard_normal((n, l))                       # p = x - er (x - yn - z / rho): above em
    below = rng.random(n) < 0.3
    below[:5] = [False, True, False, False, False][:n]
    for i in np.nonzero(below)[0]:                         # ||p|| ~ 0.3 em: exact zeros
        z[i] = rng.standard_normal(l) * 1e-4
        pt = _unit(rng, l) * em * rng.uniform(0.15, 0.45)
        if er == 1.0:
            yn[i] = pt - z[i] / RHO
        else:
            yn[i] = rng.standard_normal(l) * 1e-2
            x[i] = (pt - er * (yn[i] + z[i] / RHO)) / (1 - er)
    special = {}
    if n > 2:
        special[2] = np.zeros(l)
    if n > 3:
        special[3] = _unit(rng, l) * em * (1 + 2 * np.finfo(dt).eps)
    if n > 4:
        special[4] = _unit(rng, l) * 0.5 * THRES
    for i, pt in special.items():                          # x = yn = pt, z = 0: p = pt
        x[i] = yn[i] = pt
        z[i] = 0
        w[i] = 0
        if not pt.any():
            y[i] = atb[i] = 0
    prod = (w - RHO * yn) if form == 2 else yn
    shares = np.array([1.0])[:, None, None] if S == 1 else np.array([0.5, 0.25, 0.25])[:, None, None]
    slabs = shares * prod[None]
    if S > 1:                                              # generic rows: slabs that do not sum exactly
        generic = np.array([i not in special for i in range(n)])
        noise = rng.standard_normal((n, l)) * generic[:, None]
        slabs[0] += noise
        slabs[1] -= noise
    return tuple(np.ascontiguousarray(a.astype(dt)) for a in (slabs, x, y, z, w, atb))


def _row_reference(slabs, x, y, z, w, atb, dt, form, eta, csum=CSUM):
    """The row step in the wider type from the T inputs and T-rounded scalars, and the bars. csum:
    the depth of the fp64 accumulation (CSUM at one trip)."""
    W = _wide(dt)
    eps = float(np.finfo(dt).eps)
    u = eps / 2
    rho, er, em, tr, th = (W(dt(v)) for v in (RHO, eta * RHO, eta * MU, TAU * RHO, THRES))
    S, _, l = slabs.shape
    sw, xw, yw, zw, ww, aw = (a.astype(W) for a in (slabs, x, y, z, w, atb))
    P = np.sum(sw, axis=0)
    dP = (S - 1) * u * np.sum(np.abs(sw), axis=0)
    if form == 2:
        yn = (ww - P) / rho
        dy = dP / rho + eps * np.abs(yn)
    else:
        yn, dy = P, dP
    t1 = xw - yn
    t2 = zw / rho
    t3 = t1 - t2
    p = xw - er * t3
    dp = er * dy + u * (er * (np.abs(t1) + np.abs(t2) + 2 * np.abs(t3)) + np.abs(p))
    nr = np.sqrt(np.sum(p * p, axis=1, keepdims=True))
    dn = (l / 2 + 2) * eps * nr + np.sqrt(np.sum(dp * dp, axis=1, keepdims=True))
    c = np.maximum(nr - em, 0)
    dc = dn + u * c
    ind = nr < th
    d = ind.astype(W) + nr
    dd = dn + np.where(ind, u * d, 0)
    xn = p * c / d
    dx = (c * dp + np.abs(p) * dc) / d + np.abs(xn) * (eps + dd / d)
    r = xn - yn
    dr = dx + dy + u * np.abs(r)
    zn = zw - tr * r
    dz = tr * dr + u * (tr * np.abs(r) + np.abs(zn))
    s = yn - yw
    ds = dy + u * np.abs(s)
    a1, a2 = aw - zn, rho * xn
    wn = a1 + a2
    dw = dz + rho * dx + u * (np.abs(a1) + np.abs(a2) + np.abs(wn))
    xnorm = np.sqrt(np.sum(xn * xn, axis=1))
    dsum = np.sum(np.sqrt(np.sum(dx * dx, axis=1)) + (l / 2 + 2) * eps * xnorm) \
        + csum * np.finfo(np.float64).eps * np.sum(xnorm)
    return {"x": xn, "y": yn, "z": zn, "r": r, "s": s, "w": wn, "sum": np.sum(xnorm), "max": np.max(np.abs(xn)),
            "bx": C * dx, "by": C * dy, "bz": C * dz, "br": C * dr, "bs": C * ds, "bw": C * dw,
            "bsum": C * dsum, "bmax": C * np.max(dx),
            "at_thres": int(np.sum(np.abs(nr - th) <= C * dn)), "amb": int(np.sum(np.abs(nr - em) <= C * dn)),
            "zero_rows": (nr < em - C * dn)[:, 0], "small_rows": ((nr < th) & (nr > em + C * dn))[:, 0]}


def _step(torch, kernels, inp, form, eta):
    slabs, x, y, z, w, atb = (torch.from_numpy(a).cuda() for a in inp)
    out = kernels.admm_primal_step(slabs, x, y, z, atb, RHO, TAU, eta, MU, THRES, form=form, w=w)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _row_case(inp, dt, form, eta, pname, csum=CSUM):
    """One launch of the row kernel on ``inp`` against the wider type, then the same inputs with a
    NaN in the last row; returns the first run's outputs and the reference."""
    torch = _torch()
    from glx import kernels
    tag = "f64" if dt == np.float64 else "f32"
    S, n, l = inp[0].shape
    ref = _row_reference(*inp, dt, form, eta, csum=csum)
    where = (form, S, pname)
    assert ref["at_thres"] == 0, where      # no row at the reference's own jump
    assert ref["amb"] <= 4, where
    _note("rows at the switch", ref["amb"])
    got = _step(torch, kernels, inp, form, eta)
    for key in OUTS:
        err = np.abs(got[key].astype(_wide(dt)) - ref[key])
        bar = ref["b" + key]
        ratio = np.max(err / np.maximum(bar, np.finfo(np.float64).tiny))
        _note("%s %s" % (key, tag), ratio)
        assert np.all(err <= bar), (where, key, float(ratio))
    assert not got["x"][ref["zero_rows"]].any(), where    # rows below em: exact zeros
    if n > 1:
        assert ref["zero_rows"][1], where
    if n > 2:   # the all-zero row stays zero
        assert not any(got[key][2].any() for key in OUTS), where
    if n > 4:
        if pname == "small_eta":   # em < ||p|| < thres: non-zero through 1 + nr
            assert ref["small_rows"][4] and got["x"][4].all(), where
        else:
            assert ref["zero_rows"][4], where
    rs = abs(float(got["sums"][0]) - float(ref["sum"])) / max(float(ref["bsum"]), np.finfo(np.float64).tiny)
    rm = abs(float(got["sums"][1]) - float(ref["max"])) / max(float(ref["bmax"]), np.finfo(np.float64).tiny)
    _note("sum " + tag, rs)
    _note("max " + tag, rm)
    assert rs <= 1 and rm <= 1, (where, rs, rm)
    # the same inputs with a NaN in the last row: that row NaN, the others untouched, sums NaN
    x2 = inp[1].copy()
    x2[n - 1, l // 2] = np.nan
    got2 = _step(torch, kernels, (inp[0], x2) + inp[2:], form, eta)
    for key in ("x", "z", "r", "w"):
        assert np.isnan(got2[key][n - 1]).all(), (where, key)
    for key in OUTS:
        assert np.array_equal(got2[key][:n - 1], got[key][:n - 1]), (where, key)
    assert np.isnan(got2["sums"]).all(), where
    return got, ref


# l -> (LPR, EPL) of launch_admm_primal: 1 (1, 1), 2 (2, 1), 3 (4, 1), 5 and 8 (8, 1), 16 (16, 1),
# 17 and 32 (16, 2); 3, 5 and 17 leave lanes or a row's tail elements without a value
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("l", [1, 2, 3, 5, 8, 16, 17, 32])
@pytest.mark.parametrize("n", [1, 15, 64, 130, 257])
def test_row_kernel_against_wider_type(n, l, dt):
    small_seen = 0
    for form in (1, 2):
        for S in (1, 3):
            for pname, eta in ETAS.items():
                inp = _row_inputs(n, l, dt, form, S, eta, seed=1000 * n + 10 * l + form + S)
                _row_case(inp, dt, form, eta, pname)
                small_seen += n > 4 and pname == "small_eta"
    assert small_seen == (4 if n > 4 else 0)


def _row_inputs_large(n, l, dt, form, S, eta, seed):
    """_row_inputs for the several-trip cases, drawn in whole arrays (the same row kinds; n > 4)."""
    rng = np.random.default_rng(seed)
    er, em = eta * RHO, eta * MU
    x = rng.standard_normal((n, l))
    y = rng.standard_normal((n, l))
    z = rng.standard_normal((n, l)) * 1e-2
    w = rng.standard_normal((n, l))
    atb = rng.standard_normal((n, l))
    yn = rng.standard_normal((n, l))
    below = rng.random(n) < 0.3
    below[:5] = [False, True, False, False, False]
    below = below[:, None]
    zb = rng.standard_normal((n, l)) * 1e-4
    pt = rng.standard_normal((n, l))
    pt *= em * rng.uniform(0.15, 0.45, (n, 1)) / np.linalg.norm(pt, axis=1, keepdims=True)
    z = np.where(below, zb, z)
    if er == 1.0:
        yn = np.where(below, pt - zb / RHO, yn)
    else:
        yb = rng.standard_normal((n, l)) * 1e-2
        yn = np.where(below, yb, yn)
        x = np.where(below, (pt - er * (yb + zb / RHO)) / (1 - er), x)
    special = {2: np.zeros(l), 3: _unit(rng, l) * em * (1 + 2 * np.finfo(dt).eps), 4: _unit(rng, l) * 0.5 * THRES}
    for i, p in special.items():
        x[i] = yn[i] = p
        z[i] = 0
        w[i] = 0
    y[2] = atb[2] = 0
    prod = (w - RHO * yn) if form == 2 else yn
    shares = np.array([1.0])[:, None, None] if S == 1 else np.array([0.5, 0.25, 0.25])[:, None, None]
    slabs = shares * prod[None]
    if S > 1:
        noise = rng.standard_normal((n, l))
        noise[2:5] = 0
        slabs[0] += noise
        slabs[1] -= noise
    return tuple(np.ascontiguousarray(a.astype(dt)) for a in (slabs, x, y, z, w, atb))


# one n past a single trip of the 512-workgroup grid (512 * 256 / LPR rows) per layout: LPR 1, 2, 4,
# 8, then LPR 16 with EPL 1, a ragged EPL 2 and a full EPL 2; two trips each, the second of 5 to 8 rows
SEVERAL_TRIPS = [(1, 131077), (2, 65541), (3, 32771), (8, 16389), (16, 8200), (17, 8200), (32, 8200)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("l,n", SEVERAL_TRIPS)
def test_row_kernel_several_trips(l, n, dt):
    """Test 1 past one trip: the direct form on one slab with the default parameters, and the
    Woodbury form on three slabs with the small eta. The sum's bar is test 1's with CSUM + 1 per
    further trip: a thread adds one more row norm to its partial in each. Then the rows on both sides
    of the trip boundary run again as an input of their own, in one trip: the six outputs of a row
    depend on neither n nor the trip, so they come back bit for bit (the wrapper pre-fills them with
    NaN)."""
    torch = _torch()
    from glx import kernels
    lpr = 1
    while lpr < min(l, 16):
        lpr *= 2
    per_trip = 512 * 256 // lpr
    trips = -(-n // per_trip)
    assert trips == 2 and 0 < n - per_trip < 256 // lpr
    rows = slice(per_trip - 251, n)
    for form, S, pname in ((1, 1, "default"), (2, 3, "small_eta")):
        eta = ETAS[pname]
        inp = _row_inputs_large(n, l, dt, form, S, eta, seed=1000 * n + 10 * l + form + S)
        got, _ = _row_case(inp, dt, form, eta, pname, csum=CSUM + trips - 1)
        part = _step(torch, kernels, (np.ascontiguousarray(inp[0][:, rows]),) + tuple(a[rows].copy() for a in inp[1:]),
                     form, eta)
        for key in OUTS:
            assert np.array_equal(_bits(part[key]), _bits(got[key][rows])), (form, key)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", [1, 2], ids=["direct", "woodbury"])
@pytest.mark.parametrize("n,l", [(130, 3), (257, 32)])
def test_slab_order(n, l, form, dt):
    torch = _torch()
    from glx import kernels
    inp = _row_inputs(n, l, dt, form, 3, ETAS["small_eta"], seed=n + l)
    slabs = inp[0]
    summed = ((slabs[0] + slabs[1]) + slabs[2])[None]
    assert summed.dtype == dt and not np.array_equal(summed[0], (slabs[0] + (slabs[1] + slabs[2])))
    a = _step(torch, kernels, inp, form, ETAS["small_eta"])
    b = _step(torch, kernels, (np.ascontiguousarray(summed),) + inp[1:], form, ETAS["small_eta"])
    for key in OUTS + ("sums",):
        assert a[key].tobytes() == b[key].tobytes(), key


# ---------------------------------------------------------------------------------------------
# whole solves
# ---------------------------------------------------------------------------------------------
with open(os.path.join(GOLDEN, "admm_primal_index.json")) as _fh:
    INDEX = json.load(_fh)
CASES = sorted(INDEX)
WIDE = [c for c in CASES if INDEX[c]["m"] < INDEX[c]["n"]]


def _case(name):
    from test_admm_primal_cpu import load_case
    return load_case(name)


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - want) / np.abs(want)))


@pytest.mark.parametrize("name,form", [(c, 0) for c in CASES] + [(c, f) for c in WIDE for f in (1, 2)])
def test_solve_f64_against_reference(name, form):
    """k identical; fval, f_hist, f_hist_best within 1e-8 relative (the project's fp64 parity bar;
    the CPU restatement sits at <= 6.4e-10 direct, <= 2.1e-9 Woodbury); x within 1e-6 of max |x|;
    the counters and the resolved form as documented."""
    _torch()
    from glx import _lib, admm_primal
    from gl_ADMM_primal import gl_Admm_primal
    meta, arrs, A, b, x0, mu = _case(name)
    opts = dict(meta["opts"])
    if form:
        opts["form"] = form
    x, k, out = gl_Admm_primal(x0, A, b, mu, opts)
    fh, fb = np.asarray(out["f_hist"]), np.asarray(out["f_hist_best"])
    print(name, "form", out["glx"]["form"], "k", k, "fval rel", abs(float(out["fval"]) - float(arrs["fval"])) / float(arrs["fval"]),
          "f_hist rel", _rel(fh[:min(len(fh), len(arrs["f_hist"]))], arrs["f_hist"][:min(len(fh), len(arrs["f_hist"]))]),
          "x", float(np.max(np.abs(x - arrs["x"])) / np.max(np.abs(arrs["x"]))))
    assert k == int(arrs["k"])
    assert len(fh) == k and len(fb) == k
    _note("solve f_hist rel / 1e-8 (%s)" % out["glx"]["form"], _rel(fh, arrs["f_hist"]) / 1e-8)
    _note("solve x / 1e-6 (%s)" % out["glx"]["form"], np.max(np.abs(x - arrs["x"])) / np.max(np.abs(arrs["x"])) / 1e-6)
    assert abs(float(out["fval"]) - float(arrs["fval"])) <= 1e-8 * abs(float(arrs["fval"]))
    assert _rel(fh, arrs["f_hist"]) <= 1e-8
    assert _rel(fb, arrs["f_hist_best"]) <= 1e-8
    assert np.max(np.abs(x - arrs["x"])) <= 1e-6 * np.max(np.abs(arrs["x"]))
    g = out["glx"]
    want_form = admm_primal.FORMS[form] if form else ("Woodbury" if name in WIDE and meta["m"] ** 2 + meta["m"] * meta["n"] < meta["n"] ** 2 else "direct")
    assert g["form"] == want_form
    assert g["plan"] == _lib.admm_primal_describe(_lib.GLX_F64, meta["m"], meta["n"], meta["l"], admm_primal.make_opts(opts))
    assert g["plan"].startswith("form=%s;" % g["form"])
    assert g["syncs"] == k and g["k_calls"] == k and g["ax_calls"] == k + 1
    assert g["atr_calls"] == (k if g["form"] == "Woodbury" else 0)


def test_solve_f32_tall_direct():
    """(192, 128, 16) in float32 (m >= n, direct): x comes back float32, k identical, fval within 1e-4
    relative (the project's fp32 bar; the CPU emulation sits at 9.8e-8)."""
    _torch()
    from gl_ADMM_primal import gl_Admm_primal
    meta, arrs, A, b, x0, mu = _case("admm_primal_192x128x16")
    x, k, out = gl_Admm_primal(x0.astype(np.float32), A.astype(np.float32), b.astype(np.float32), mu, {})
    print("f32 k", k, "fval rel", abs(float(out["fval"]) - float(arrs["fval"])) / float(arrs["fval"]))
    _note("solve f32 fval rel / 1e-4", abs(float(out["fval"]) - float(arrs["fval"])) / float(arrs["fval"]) / 1e-4)
    assert x.dtype == np.float32 and out["glx"]["form"] == "direct"
    assert k == int(arrs["k"])
    assert abs(float(out["fval"]) - float(arrs["fval"])) <= 1e-4 * abs(float(arrs["fval"]))


@pytest.mark.parametrize("name", WIDE)
def test_solve_f32_wide_is_refused(name, monkeypatch):
    """m < n in float32 raises in every form, before the setup is spent or anything is launched."""
    _torch()
    from glx import _lib, admm_primal
    meta, arrs, A, b, x0, mu = _case(name)

    def _no_setup(*a, **k):
        raise AssertionError("the setup ran")
    monkeypatch.setattr(admm_primal, "setup", _no_setup)
    monkeypatch.setattr(admm_primal, "workspace", _no_setup)
    for form in (0, 1, 2):
        with pytest.raises(_lib.GlxError, match="condition") as e:
            admm_primal.solve(x0.astype(np.float32), A.astype(np.float32), b.astype(np.float32), mu, {"form": form})
        assert e.value.code == 1   # GLX_E_INVALID


def test_options_and_determinism():
    """(128, 256, 32) fp64: a repeat gives the same bits; maxit, thres, converge_len, rho, tau, eta_0
    and step_type reach the solver, in both forms where they change the arithmetic."""
    _torch()
    from glx import admm_primal
    import admm_primal_ref
    meta, arrs, A, b, x0, mu = _case("admm_primal_128x256x32")
    x1, k1, o1 = admm_primal.solve(x0, A, b, mu, {})
    x2, k2, o2 = admm_primal.solve(x0, A, b, mu, {})
    assert k1 == k2 == int(arrs["k"])
    assert np.array_equal(x1, x2) and o1["f_hist"] == o2["f_hist"]
    # a short maxit ends with k = maxit
    xs, ks, os_ = admm_primal.solve(x0, A, b, mu, {"maxit": 3})
    assert ks == 3 and len(os_["f_hist"]) == 3 and os_["f_hist"] == o1["f_hist"][:3]
    assert os_["fval"] == os_["f_hist"][-1]
    # converge_len and thres: with a huge thres every iteration counts, so k = converge_len
    _, kc, _ = admm_primal.solve(x0, A, b, mu, {"thres": 1e30, "converge_len": 5})
    assert kc == 5
    for o in ({"rho": 5e-2}, {"tau": 1.0}, {"eta_0": 50}, {"step_type": "diminishing"},
              {"step_type": "diminishing2"}, {"step_type": "fixed", "form": 1}, {"rho": 5e-2, "form": 1}):
        o = {"maxit": 4, **o}
        _, kg, got = admm_primal.solve(x0, A, b, mu, o)
        _, kw, want = admm_primal_ref.gl_admm_primal(x0, A, b, mu, o)
        assert kg == kw == 4
        if "form" not in o and o.get("step_type") != "fixed":
            assert got["f_hist"] != o1["f_hist"][:4], o
        print(o, "f_hist rel", _rel(got["f_hist"], np.asarray(want["f_hist"])))
        assert _rel(got["f_hist"], np.asarray(want["f_hist"])) <= 1e-8, o
    # maxit = 0: no iteration, the objective of x0
    x0c, k0, o0 = admm_primal.solve(x0, A, b, mu, {"maxit": 0})
    assert k0 == 0 and o0["f_hist"] == [] and np.array_equal(x0c, x0)
    f0 = 0.5 * np.sum((A @ x0 - b) ** 2) + mu * np.sum(np.linalg.norm(x0, axis=1))
    assert abs(float(o0["fval"]) - f0) <= 1e-10 * f0
    assert o0["glx"]["ax_calls"] == 1 and o0["glx"]["syncs"] == 0 and o0["glx"]["k_calls"] == 0


def test_drop_in_module_contract(caplog):
    """gl_ADMM_primal.gl_Admm_primal on the default instance with NumPy arrays: NumPy out, x0 and
    the caller's opts untouched, the reference's keys, its debug lines."""
    import logging
    torch = _torch()
    from gl_ADMM_primal import gl_Admm_primal
    meta, arrs, A, b, x0, mu = _case("admm_primal_256x512x2")
    x0_before = x0.copy()
    opts = {"maxit": 10, "not_an_option": 1, "converge_thres": 1e-5}
    opts_before = dict(opts)
    with caplog.at_level(logging.DEBUG, logger="opt"):
        x, k, out = gl_Admm_primal(x0, A, b, mu, opts)
    lines = [r.getMessage() for r in caplog.records if r.name == "opt"]
    assert len(lines) == 10 and lines[0].startswith("iter=     1, objective=") and "sparsity=" in lines[0]
    assert isinstance(x, np.ndarray) and x.dtype == np.float64 and x.shape == x0.shape
    assert isinstance(k, int) and k == 10
    assert np.array_equal(x0, x0_before) and opts == opts_before
    assert {"tt", "fval", "f_hist", "f_hist_best", "glx"} <= set(out)
    assert {"setup_s", "loop_s", "form", "k_calls", "ax_calls", "atr_calls", "syncs", "plan"} <= set(out["glx"])
    assert out["tt"] >= out["glx"]["setup_s"] > 0
    assert np.allclose(out["f_hist"], arrs["f_hist"][:10], rtol=1e-8, atol=0)
    # torch in, torch out
    xt, kt, outt = gl_Admm_primal(torch.from_numpy(x0).cuda(), torch.from_numpy(A).cuda(),
                                  torch.from_numpy(b).cuda(), mu, opts)
    assert isinstance(xt, torch.Tensor) and kt == 10 and np.array_equal(xt.cpu().numpy(), x)
