"""The descent-method kernels, one launch at a time, against a plain NumPy reference.

What SGD, GD and FGD run between the dense products: k_descent, k_fgd_grad, k_rownorm_max,
k_count_above, k_threshold, k_thr_axpby (kernels_elem.hip), and the one-pass kernel of an l = 1
descent iteration, k_gemv_pair_fused with k_sum_cols (kernels_gemv.hip). Reached here through
glx_descent_step, glx_fgd_gradient, glx_row_stats, glx_threshold, glx_thr_combine and
glx_descent_pass (glx.kernels); no session, no solve.

Reference: the formulas as the reference project states them (SGD gl_SGD_primal.py:56-61, 93-96;
GD gl_GD_primal.py:59-63, 95-98; FGD gl_FGD_primal.py:64-72, 139-142), written below in NumPy
(nothing imported from glx), with the scalars rounded to the kernel's type T first, as the
launchers do: alpha, mu, thres, delta, delta * delta (formed in double, then rounded), 1e-6, a, b.

Three tiers of bars; none is fitted to the kernel.

(a) Bit identity with NumPy in T. The library is built with -ffp-contract=off, and / and sqrt are
correctly rounded in both types, so where kernel and NumPy do the same IEEE operations in the same
order every bit agrees:
  glx_threshold    xo (aliased and out of place): |v| == thres kept, -0.0 -> +0.0, NaN copied;
                   *flag == epoch iff a nonzero value was zeroed, else the sentinel it held.
  glx_thr_combine  xk = thr(xk), y = a thr(xk) + b vk (two products, one sum).
  glx_row_stats    max == np.abs(x).max() (NaN with a NaN present); count ==
                   np.sum(np.abs(x) > T(1e-6) * T(max)) in T (0 with a NaN): one rounded product of an
                   exact maximum, so no ambiguity set.
  glx_descent_step, glx_fgd_gradient at l in {1, 2}: the row norm is sqrt(x0 x0 [+ x1 x1]) in
                   both, so x, xt and g equal the reference lines evaluated in T.
  fh[0] of the pass == 0.5 * sums[0] + fh_mu * rn in Python doubles from the returned sums[0].

(b) eps bars for the row kernels (every l; the reference in np.longdouble for f64 inputs and
np.float64 for f32 inputs; eps = T's machine epsilon, u = eps / 2 the unit roundoff). Term by term:
  d        the row sum s holds l squares (1 u each) under <= 12 additions (8 in a lane, 4 shuffle
           levels): relative 13 u, 14 u with GD's / FGD's + delta^2; the root halves that and adds
           its own: <= 8 u; SGD's + (nrm < thres) one more: d carries <= 8.5 u = 4.25 eps.
  x_new    q = xt / d: 9.5 u; mu q: 10.5 u; g + mu q rounds once: u (|g| + mu |q|); alpha (..) once
           more; the last subtraction u |x_new| <= u (|xt| + alpha (|g| + mu |q|)). Together
           <= 13.5 u (|xt| + alpha (|g| + mu |q|)), and the bar is
             |x_new - ref| <= B = 16 eps (|xt| + alpha (|g| + mu |q|)) + alpha (S - 1) eps sum_k |g_k|
           (the slab sum's S - 1 additions enter through g and are scaled by alpha with it).
  xt_out   thr(x_new): equal to thr of the returned x everywhere (one compare in T), and to the
           reference's decision outside the ambiguity set.
  sum      sum_i ||x_new_i||: sum_i (||B_i||_2 + 8 eps ||x_new_i||) (triangle inequality, then the
           squares, their additions and the root, as for d) + CSUM eps64 sum |term| for the fp64
           accumulation (<= CSUM = 32 additions deep: a few per thread, 8 levels in the workgroup,
           12 over the workgroup partials).
  g (FGD)  |g - ref| <= 16 eps (|gp| + mu |y| / d) + (S - 1) eps sum_k |gp_k| (y / d: 9 u, mu (..):
           10 u, the sum: u (|gp| + mu |y| / d), the slab sum as above, unscaled).
  smooth   sum_i (d_i - delta): per row 8 eps d_i: the bound is in d, not in d - delta, because the
           subtraction cancels for ||y|| << delta (d carries 4 eps d, the subtraction eps / 2 of a
           result <= d); + CSUM eps64 sum |term|.
  row sum  glx_row_stats' sum_i ||x_i||: sum_i 8 eps ||x_i|| + CSUM eps64 sum |term|.
The ambiguity set of a case: the elements with ||x_new| - thres| <= B and, in mode 0, the rows with
| ||xt|| - thres | <= 16 eps ||xt|| (d may take the other denominator there). A case whose set
holds more than 4 members fails; every case below has 0: a case takes the first of its seeds
whose set, counted on the CPU from the reference alone, is empty, and asserts that again.

(c) The one-pass kernel. r1 = A x - b and r2 = A thr(x) - b are not outputs, so their error is
propagated. With E = 16 / sizeof(T) elements per 16-byte vector, VPT = ceil(n / E / 512) rounded up
to 1 / 2 / 4 / 8 vectors per thread:
  delta_i   = (VPT E + 2) eps (sum_j |a_ij| |x_j| + |b_i|): the thread's sequential chain of VPT E
              products in T; the rest of the dot product is fp64; one rounding to T, one subtraction.
  G         |G - Gref|_j <= sum_i |a_ij| delta_i + (ceil(m / blocks) + ceil(blocks / 4) + 4) eps
              sum_i |a_ij| |r2_i|: a workgroup adds its rows in order, a wave of k_sum_cols a quarter
              of the slabs, then three more additions; the product rounds once.
  sums[k]   sum_i (2 |r_i| delta_i + delta_i^2) + (ceil(m / blocks) + 16) eps64 sum r_i^2.
The reference r and G are computed in the wider type from the same T inputs. nt = 0 and nt = 1
give the same bits, and so do two runs. Shapes the kernel does not take (n no multiple of E, more
than 8 vectors per thread) return GLX_E_INVALID with a message and write nothing.

Every row case carries one all-zero row (xt / y and g), one row holding -0.0, one row of norm
below thres (mode 0's + 1 denominator), one row of norm ~ 1e-3 delta and one row holding a NaN.
The NaN would turn the sum into NaN, so each case runs twice: with a finite value in place of the
NaN (all the bars above), and with the NaN (every other row bit-identical to the first run, the
row itself NaN, the sum NaN).

Measured on an MI355X, worst error / bound over all cases of this file (f64, f32); the module
prints the table and the ambiguity sets' sizes when its tests are over (pytest -s):
  x_new          0.123  0.123      sum |x_new_i|  0.0183 0.0208     g (FGD)        0.123  0.123
  sum smooth     0.0332 0.0622     sum |x_i|      0.0212 0.0561     G (pass)       0.117  0.0364
  sum r1^2       0.0557 0.0187     sum r2^2       0.0319 0.00095
None is above 1. One is just below 1e-3 (sum r2^2 in f32, the largest of six cases; its bar lets
the roundings of every row's chain add up with one sign, while sum r1^2 under the same bar sits at
0.019); the others are not, so the constants stand as derived. Every tier (a) comparison held bit
for bit.
Ambiguity sets: 0 members in every case (largest set 0 over the 464 references built).

The row kernels' cases by layout (dispatch_row: LPR lanes per row = the power of two >= l up to 16,
then EPL = ceil(l / 16) elements per lane at LPR 16). LS selects (LPR, EPL) =
  l = 1 (1, 1)   2 (2, 1)   3 (4, 1)   8 (8, 1)   16 (16, 1)   17, 32 (16, 2)   40 (16, 3)
  64 (16, 4)   72 (16, 5)   88 (16, 6)   104 (16, 7)   128 (16, 8)
which is every instantiation of k_descent, k_fgd_grad and k_rownorm_max, at one trip; MULTI_TRIP
makes two trips at LPR 1, 2, 4, 8 and at LPR 16 with EPL 1 and 8.

What a one-line slip would trip (each tried on a NumPy model of the kernels' arithmetic put in
place of the library, never as device code):
  the `(nrm < thres)` term dropped from d              test_descent_step, _several_trips (mode 0: the
                                                      all-zero row is NaN, the row below thres off)
  delta for delta^2                                   test_descent_step, _several_trips (mode 1),
                                                      test_fgd_gradient, _several_trips
  d for d - delta in the smoothed norm                `sum smooth` in test_fgd_gradient, _several_trips
  the tail lanes j >= l of l = 17 entering a row sum  test_descent_step, test_fgd_gradient,
                                                      test_row_stats (each at l = 17)
  `>=` for `>` in the count                           test_row_stats_count_is_strict
  `<=` for `<` in the threshold                       test_threshold, test_threshold_flag_keeps_sentinel,
                                                      test_thr_combine, test_descent_threshold_edge_is_strict
  the last slab dropped in the column sum             G in test_descent_pass (every shape)
  e1 for e2 in the rank-1 update                      G in test_descent_pass (every shape)
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALPHA, THRES, DELTA = 0.05, 1e-3, 1e-4
MUS = (0.02, 2e-4)
THETA = 2.0 / 7.0
FH_MU = 0.013
CSUM = 32
EPS64 = float(np.finfo(np.float64).eps)
MAX_AMBIGUOUS = 4
# l -> (lanes per row, elements per lane) of dispatch_row: 1 (1, 1), 2 (2, 1), 3 (4, 1), 8 (8, 1),
# 16 (16, 1), 17 and 32 (16, 2), 40 (16, 3), 64 (16, 4), 72 (16, 5), 88 (16, 6), 104 (16, 7), 128 (16, 8)
LS = [1, 2, 3, 8, 16, 17, 32, 40, 64, 72, 88, 104, 128]
# one n past a single trip of 512 workgroups (512 * 256 / LPR rows) per lanes-per-row layout
MULTI_TRIP = [(1, 131077), (2, 65541), (3, 32771), (8, 16389), (16, 8200), (128, 8200)]
FLAT_COUNTS = [1, 255, 1025, 1024 * 1024 + 128]   # the last passes the 1024-workgroup cap

# worst error / bound per (output, dtype) and the ambiguity sets' sizes, printed when the module's
# tests are over (pytest -s)
RATIOS = {}
AMBIGUOUS = {"references": 0, "largest set": 0, "members in all": 0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(RATIOS):
        print("ratio %-14s %s  %.3e" % (key[0], key[1], RATIOS[key]))
    print("ambiguity sets:", AMBIGUOUS)


def _k():
    from glx import kernels
    return kernels


def _types(dtype):
    return (np.float64, np.longdouble) if dtype == "f64" else (np.float32, np.float64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def _out_np(o):
    return {k: _np(v) for k, v in o.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b, where=None):
    eq = _bits(a) == _bits(b)
    return bool(eq.all() if where is None else eq[where].all())


def _same_bits_nan(got, want):
    """Equal bits wherever the expectation is a number, a NaN (of any payload) where it is not."""
    return np.array_equal(np.isnan(got), np.isnan(want)) and _same_bits(got, want, ~np.isnan(want))


def _note(name, dtype, r):
    RATIOS[(name, dtype)] = max(RATIOS.get((name, dtype), 0.0), r)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _gen(n, l, dtype, seed, S=1):
    """Rows of x at four scales (a quarter all-zero), rows of g at four, g in S slabs."""
    npdt = _types(dtype)[0]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, l)) * rng.choice([0, 1e-3, 3e-2, 1.0], (n, 1), p=[.25, .25, .3, .2])
    g = rng.standard_normal((S, n, l)) * rng.choice([1e-4, 1e-2, 1.0, 30.0], (n, 1))
    return x.astype(npdt), g.astype(npdt)


def _special_rows(x, g):
    """Row n-1 = -0.0 in x (and one -0.0 in g), row n-3 all zero (x and g), row n-4 of norm
    ~ thres / 4, row n-5 of norm ~ 1e-3 delta; returns where the NaN variant puts its NaN (row
    n-2). g is (S, n, l)."""
    n, l = x.shape
    rng = np.random.default_rng(n + l)
    x[n - 5] = (1e-3 * DELTA / math.sqrt(l)) * rng.standard_normal(l)
    x[n - 4] = (0.25 * THRES / math.sqrt(l)) * rng.choice([-1.0, 1.0], l) * rng.uniform(0.5, 1.0, l)
    x[n - 3] = 0.0
    x[n - 1] = -0.0
    g[:, n - 3] = 0.0
    g[:, n - 1, 0] = -0.0
    return n - 2, l // 2


def _with_nan(x, pos):
    xn = x.copy()
    xn[pos] = np.nan
    return xn


def _hand_values(npdt):
    th = npdt(THRES)
    tiny = np.nextafter(npdt(0), npdt(1))
    vals = [th, -th, np.nextafter(th, npdt(0)), np.nextafter(th, npdt(np.inf)), npdt(0.0), npdt(-0.0), tiny,
            npdt(np.inf), npdt(np.nan), -np.nextafter(th, npdt(0)), -np.nextafter(th, npdt(np.inf)), -tiny,
            npdt(-np.inf), npdt(0.5)]
    return np.array(vals, dtype=npdt)


def _flat_input(count, dtype, seed):
    """count values: the threshold's edge values where they fit, then values at the row scales."""
    npdt = _types(dtype)[0]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(count) * rng.choice([0, 1e-4, 1e-3, 3e-2, 1.0], count)).astype(npdt)
    vals = _hand_values(npdt)
    if count > 4 * vals.size:
        x[rng.choice(count, 4 * vals.size, replace=False)] = np.tile(vals, 4)
    return x


# ---------------------------------------------------------------------------------------------
# the reference (plain NumPy): C = the compute type, the kernel's T for tier (a), one step wider
# for tier (b)
# ---------------------------------------------------------------------------------------------
def _slab_sum(g, C):
    s = g[0].astype(C)
    for k in range(1, g.shape[0]):
        s = s + g[k].astype(C)
    return s


def descent_lines(xt, g, alpha, mu, thres, delta, mode, C):
    """gl_SGD_primal.py:56-61, 93-96 (mode 0) / gl_GD_primal.py:59-63, 95-98 (mode 1) on the
    thresholded iterate xt, in the type C; g = the slabs' sum in slab order."""
    T = xt.dtype.type
    al, m_, th, dd = C(T(alpha)), C(T(mu)), C(T(thres)), C(T(delta * delta))
    X, Gs = xt.astype(C), _slab_sum(g, C)
    s = (X * X).sum(axis=1, keepdims=True)
    nrm = np.sqrt(s)
    with np.errstate(invalid="ignore"):
        d = (nrm < th).astype(C) + nrm if mode == 0 else np.sqrt(s + dd)
        q = X / d
        xn = X - al * (Gs + m_ * q)
        small = np.abs(xn) < th
    return dict(x=xn, xt=np.where(small, C(0), xn), small=small, nrm=nrm, q=q, g=Gs, al=al, mu=m_, th=th)


def ref_descent(xt, g, alpha, mu, thres, delta, mode):
    T, C = xt.dtype.type, (np.longdouble if xt.dtype == np.float64 else np.float64)
    eps = C(np.finfo(T).eps)
    r = descent_lines(xt, g, alpha, mu, thres, delta, mode, C)
    S = g.shape[0]
    B = 16 * eps * (np.abs(xt.astype(C)) + r["al"] * (np.abs(r["g"]) + r["mu"] * np.abs(r["q"])))
    B = B + r["al"] * (S - 1) * eps * np.abs(g.astype(C)).sum(axis=0)
    amb_e = np.abs(np.abs(r["x"]) - r["th"]) <= B
    amb_r = np.zeros(xt.shape[0], dtype=bool)
    if mode == 0:
        amb_r = (np.abs(r["nrm"] - r["th"]) <= 16 * eps * r["nrm"])[:, 0]
    xnn = np.sqrt((r["x"] * r["x"]).sum(axis=1))
    # a row on the ||xt|| = thres step may take the other denominator: its norm moves by <= alpha mu
    sbnd = (np.sqrt((B * B).sum(axis=1)) + 8 * eps * xnn).sum() + CSUM * EPS64 * xnn.sum() \
        + r["al"] * r["mu"] * amb_r.sum()
    r.update(B=B, amb_e=amb_e, amb_r=amb_r, sum=xnn.sum(), sbnd=sbnd)
    return r


def fgd_lines(y, gp, mu, delta, C):
    """gl_FGD_primal.py:64-72 in the type C."""
    T = y.dtype.type
    m_, dd, dl = C(T(mu)), C(T(delta * delta)), C(T(delta))
    Y, Gs = y.astype(C), _slab_sum(gp, C)
    d = np.sqrt((Y * Y).sum(axis=1, keepdims=True) + dd)
    return dict(g=Gs + m_ * (Y / d), d=d, term=d - dl, gp=Gs, mu=m_)


def ref_fgd(y, gp, mu, delta):
    T, C = y.dtype.type, (np.longdouble if y.dtype == np.float64 else np.float64)
    eps = C(np.finfo(T).eps)
    r = fgd_lines(y, gp, mu, delta, C)
    S = gp.shape[0]
    B = 16 * eps * (np.abs(r["gp"]) + r["mu"] * np.abs(y.astype(C)) / r["d"])
    B = B + (S - 1) * eps * np.abs(gp.astype(C)).sum(axis=0)
    r.update(B=B, sum=r["term"].sum(), sbnd=(8 * eps * r["d"]).sum() + CSUM * EPS64 * np.abs(r["term"]).sum())
    return r


def thr_T(x, thres):
    """x[np.abs(x) < thres] = 0 in x's own type (gl_SGD_primal.py:93)."""
    T = x.dtype.type
    small = np.abs(x) < T(thres)
    return np.where(small, T(0), x), small


def ref_pass(A, x, xt, b, blocks):
    """r1 = A x - b, r2 = A xt - b, G = A^T r2 and the two sums in the wider type, with the bars
    of tier (c)."""
    T, C = A.dtype.type, (np.longdouble if A.dtype == np.float64 else np.float64)
    eps = C(np.finfo(T).eps)
    m, n = A.shape
    E = 16 // A.dtype.itemsize
    vpt = -(-n // (E * 512))
    vpt = [v for v in (1, 2, 4, 8) if v >= vpt][0]
    Ac, bc = A.astype(C), b.astype(C)
    absA = np.abs(Ac)
    rs, dl, sums, sbnd = [], [], [], []
    rows = -(-m // blocks)
    for v in (x, xt):
        vc = v.astype(C)
        r = Ac @ vc - bc
        d = (vpt * E + 2) * eps * (absA @ np.abs(vc) + np.abs(bc))
        rs.append(r)
        dl.append(d)
        sums.append((r * r).sum())
        sbnd.append((2 * np.abs(r) * d + d * d).sum() + (rows + 16) * EPS64 * (r * r).sum())
    G = Ac.T @ rs[1]
    BG = absA.T @ dl[1] + (rows + -(-blocks // 4) + 4) * eps * (absA.T @ np.abs(rs[1]))
    return dict(G=G, BG=BG, sums=sums, sbnd=sbnd, vpt=vpt)


# ---------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------
def _check_close(name, dtype, got, ref, bound, skip=None):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), name
    v = ~np.isnan(ref)
    if skip is not None:
        v = v & ~skip
    err = np.abs(got.astype(ref.dtype) - ref)
    assert not (err[v & (bound == 0)] != 0).any(), name
    nz = v & (bound > 0)
    r = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    _note(name, dtype, r)
    assert r <= 1.0, (name, dtype, r)


def _check_sum(name, dtype, got, ref, bound):
    err = abs(np.longdouble(got) - np.longdouble(ref))
    bound = np.longdouble(bound)
    r = float(err / bound) if bound > 0 else (0.0 if err == 0 else np.inf)
    _note(name, dtype, r)
    assert r <= 1.0, (name, dtype, r, float(got), float(ref))


def _amb_count(ref):
    c = int(ref["amb_e"].sum()) + int(ref["amb_r"].sum())
    AMBIGUOUS["references"] += 1
    AMBIGUOUS["largest set"] = max(AMBIGUOUS["largest set"], c)
    AMBIGUOUS["members in all"] += c
    assert c <= MAX_AMBIGUOUS, "ambiguity set holds %d members" % c
    return c


def run_descent(xt, g, mu, mode):
    return _out_np(_k().descent_step(_dev(xt), _dev(g), ALPHA, mu, THRES, DELTA, mode))


def run_fgd(y, gp, mu):
    return _out_np(_k().fgd_gradient(_dev(y), _dev(gp), mu, DELTA))


def descent_inputs(n, l, dtype, S, mu, mode, seed):
    """The case's inputs and reference: the first of the seeds seed, seed + 100003, ... whose
    ambiguity set, counted from the reference alone, is empty (with f32 and 10^5 .. 10^6 elements
    about one seed in two leaves an element within B of thres)."""
    for k in range(16):
        xt, g = _gen(n, l, dtype, seed + 100003 * k, S=S)
        nanpos = _special_rows(xt, g)
        ref = ref_descent(xt, g, ALPHA, mu, THRES, DELTA, mode)
        if not (ref["amb_e"].any() or ref["amb_r"].any()):
            return xt, g, nanpos, ref
    raise AssertionError("no seed with an empty ambiguity set")


def descent_case(dtype, xt, g, mu, mode, nanpos, ref):
    """Both variants of one SGD / GD case with all its checks."""
    T = xt.dtype.type
    out = run_descent(xt, g, mu, mode)
    assert _amb_count(ref) == 0
    skip = ref["amb_r"][:, None] | np.zeros(xt.shape, dtype=bool)
    _check_close("x_new", dtype, out["x"], ref["x"], ref["B"], skip)
    want, _ = thr_T(out["x"], THRES)
    assert _same_bits(out["xt"], want), "xt_out is thr of the returned x"
    ok = ~(ref["amb_e"] | skip)
    assert _same_bits(out["xt"], np.where(ref["small"], T(0), out["x"]), ok), "xt_out, the reference's decision"
    _check_sum("sum |x_new_i|", dtype, out["sum"][0], ref["sum"], ref["sbnd"])
    if xt.shape[1] <= 2:   # tier (a): the same IEEE operations in the same order
        line = descent_lines(xt, g, ALPHA, mu, THRES, DELTA, mode, T)
        assert line["x"].dtype == xt.dtype
        assert _same_bits(out["x"], line["x"]) and _same_bits(out["xt"], line["xt"]), "bit identity, l <= 2"
    nan = run_descent(_with_nan(xt, nanpos), g, mu, mode)
    rows = np.arange(xt.shape[0]) != nanpos[0]
    for key in ("x", "xt"):
        assert _same_bits(out[key][rows], nan[key][rows]), key
        assert np.isnan(nan[key][nanpos[0]]).all(), key
    assert np.isnan(nan["sum"][0])
    return out, ref


def fgd_case(dtype, y, gp, mu, nanpos):
    T = y.dtype.type
    out = run_fgd(y, gp, mu)
    ref = ref_fgd(y, gp, mu, DELTA)
    _check_close("g (FGD)", dtype, out["g"], ref["g"], ref["B"])
    _check_sum("sum smooth", dtype, out["sum"][0], ref["sum"], ref["sbnd"])
    if y.shape[1] <= 2:
        line = fgd_lines(y, gp, mu, DELTA, T)
        assert line["g"].dtype == y.dtype and _same_bits(out["g"], line["g"]), "bit identity, l <= 2"
    nan = run_fgd(_with_nan(y, nanpos), gp, mu)
    rows = np.arange(y.shape[0]) != nanpos[0]
    assert _same_bits(out["g"][rows], nan["g"][rows])
    assert np.isnan(nan["g"][nanpos[0]]).all() and np.isnan(nan["sum"][0])
    return out, ref


# ---------------------------------------------------------------------------------------------
# row kernels: every lanes-per-row / elements-per-lane instantiation, one and several workgroups
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
def test_descent_step(mode, dtype, l, n, mu, S):
    xt, g, nanpos, ref = descent_inputs(n, l, dtype, S, mu, mode, seed=1000 * l + n + 7)
    descent_case(dtype, xt, g, mu, mode, nanpos, ref)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("l,n", MULTI_TRIP)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", [0, 1])
def test_descent_step_several_trips(mode, dtype, l, n, S):
    mu = MUS[(l + S + mode) % 2]
    xt, g, nanpos, ref = descent_inputs(n, l, dtype, S, mu, mode, seed=1000 * l + n + 7)
    descent_case(dtype, xt, g, mu, mode, nanpos, ref)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fgd_gradient(dtype, l, n, mu, S):
    y, gp = _gen(n, l, dtype, seed=1000 * l + n + 11, S=S)
    nanpos = _special_rows(y, gp)
    _, ref = fgd_case(dtype, y, gp, mu, nanpos)
    assert 0 < ref["term"][n - 5, 0] < 1e-5 * DELTA      # the row where d - delta cancels


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("l,n", MULTI_TRIP)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fgd_gradient_several_trips(dtype, l, n, S):
    y, gp = _gen(n, l, dtype, seed=1000 * l + n + 11, S=S)
    nanpos = _special_rows(y, gp)
    fgd_case(dtype, y, gp, MUS[(l + S) % 2], nanpos)


@pytest.mark.parametrize("l", [1, 16])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_descent_threshold_edge_is_strict(dtype, l):
    """Rows of xt with one nonzero entry x0 within 8 ulps of +-thres, g = 0 and mu = 0: then
    x_new = x0 - alpha * (0 + 0 * (x0 / d)) = x0 exactly for any finite d > 0, and thr keeps
    |x0| >= thres (the compare is np.abs(x) < thres, gl_SGD_primal.py:93), zeroes the rest."""
    T = _types(dtype)[0]
    th = T(THRES)
    x0 = [th]
    for _ in range(8):
        x0 = [np.nextafter(x0[0], T(0))] + x0 + [np.nextafter(x0[-1], T(1))]
    x0 = np.array(x0 + [-v for v in x0], dtype=T)
    xt = np.zeros((x0.size, l), dtype=T)
    xt[:, l // 2] = x0
    g = np.zeros((1,) + xt.shape, dtype=T)
    want, small = thr_T(xt, THRES)
    assert (np.abs(x0) == th).any() and small[:, l // 2].any() and (~small[:, l // 2]).any()
    for mode in (0, 1):
        o = run_descent(xt, g, 0.0, mode)
        assert _same_bits(o["x"], xt) and _same_bits(o["xt"], want), mode
        assert o["sum"][0] == pytest.approx(float(np.abs(x0).astype(np.float64).sum()), rel=1e-14), mode


# ---------------------------------------------------------------------------------------------
# row-norm sum, maximum and the count that reads it
# ---------------------------------------------------------------------------------------------
def _row_stats_case(dtype, x, nanpos):
    T, C = _types(dtype)
    eps = C(np.finfo(T).eps)
    s = _np(_k().row_stats(_dev(x))["stats"])
    mx = np.abs(x).max()
    assert s[1] == float(mx), "max |x|"
    assert s[2] == float(np.sum(np.abs(x) > T(1e-6) * T(mx))), "count above 1e-6 max"
    assert 0 < s[2] < x.size
    nr = np.sqrt((x.astype(C) ** 2).sum(axis=1))
    _check_sum("sum |x_i|", dtype, s[0], nr.sum(), (8 * eps * nr).sum() + CSUM * EPS64 * nr.sum())
    sn = _np(_k().row_stats(_dev(_with_nan(x, nanpos)))["stats"])
    assert np.isnan(sn[0]) and np.isnan(sn[1]) and sn[2] == 0.0


@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_row_stats(dtype, l, n):
    x, g = _gen(n, l, dtype, seed=1000 * l + n + 13)
    _row_stats_case(dtype, x, _special_rows(x, g))


@pytest.mark.parametrize("l,n", MULTI_TRIP + [(128, 8193)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_row_stats_several_trips(dtype, l, n):
    """(128, 8193): 1024 * 1024 + 128 values, past the count's 1024-workgroup cap."""
    x, g = _gen(n, l, dtype, seed=1000 * l + n + 13)
    _row_stats_case(dtype, x, _special_rows(x, g))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_row_stats_count_is_strict(dtype):
    """|x| == T(1e-6) * T(max) is not counted (sparsity_func: np.abs(x) > 1e-6 * max)."""
    T = _types(dtype)[0]
    edge = T(1e-6) * T(0.75)
    x = np.zeros((40, 3), dtype=T)
    x[0, 1] = T(-0.75)
    x[3:9, 2] = [edge, -edge, np.nextafter(edge, T(1)), -np.nextafter(edge, T(1)), np.nextafter(edge, T(0)), T(-0.0)]
    s = _np(_k().row_stats(_dev(x))["stats"])
    assert s[1] == 0.75 and s[2] == 3.0


# ---------------------------------------------------------------------------------------------
# flat kernels
# ---------------------------------------------------------------------------------------------
SENTINEL = -77


def _run_threshold(x, inplace, epoch):
    flag = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    o = _k().threshold(_dev(x), THRES, flag=flag, epoch=epoch, inplace=inplace)
    return _np(o["xo"]), int(_np(o["flag"])[0])


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("count", FLAT_COUNTS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_threshold(dtype, count, inplace):
    x = _flat_input(count, dtype, seed=count)
    if count == 1:
        x[0] = 0.25 * THRES
    want, small = thr_T(x, THRES)
    assert (small & (x != 0)).any()
    xo, flag = _run_threshold(x, inplace, epoch=5 + count % 7)
    assert _same_bits(xo, want)           # NaN copied bit for bit, -0.0 -> +0.0, |v| == thres kept
    assert flag == 5 + count % 7
    # the output is a fixed point: nothing nonzero is left to zero, so the flag keeps its sentinel
    xo2, flag2 = _run_threshold(want, inplace, epoch=9)
    assert _same_bits(xo2, want) and flag2 == SENTINEL


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("count", FLAT_COUNTS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_threshold_flag_keeps_sentinel(dtype, count, inplace):
    T = _types(dtype)[0]
    zero = np.zeros(count, dtype=T)
    xo, flag = _run_threshold(zero, inplace, epoch=3)
    assert _same_bits(xo, zero) and flag == SENTINEL
    # only -0.0 lies below thres: it becomes +0.0, and that is no change
    x = np.full(count, T(0.5))
    x[:: 3] = T(-0.0)
    if count > 1:
        x[count // 2] = T(THRES)
    want, _ = thr_T(x, THRES)
    assert np.signbit(x).any() and not np.signbit(want).any()
    xo, flag = _run_threshold(x, inplace, epoch=3)
    assert _same_bits(xo, want) and flag == SENTINEL


@pytest.mark.parametrize("count", FLAT_COUNTS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_thr_combine(dtype, count):
    T = _types(dtype)[0]
    xk = _flat_input(count, dtype, seed=count + 1)
    vk = _flat_input(count, dtype, seed=count + 2)
    a, b = T(1.0 - THETA), T(THETA)
    xo, _ = thr_T(xk, THRES)
    with np.errstate(all="ignore"):
        y = a * xo + b * vk
    assert y.dtype == xk.dtype
    o = _out_np(_k().thr_combine(_dev(xk), _dev(vk), THRES, 1.0 - THETA, THETA))
    assert _same_bits(o["xk"], xo)
    assert _same_bits_nan(o["y"], y)


# ---------------------------------------------------------------------------------------------
# the one-pass kernel of an l = 1 descent iteration
# ---------------------------------------------------------------------------------------------
PASS_F64 = [(m, 64) for m in range(1, 10)] + [(m, 4098) for m in range(1, 10)] + \
    [(7, 2), (9, 1024), (13, 1026), (37, 2050), (17, 8192), (33, 512), (2049, 64), (3001, 1030)]
PASS_F32 = [(7, 4), (9, 2048), (13, 2052), (21, 8196), (5, 16384), (3001, 1028)]
PASS_CASES = [("f64",) + s for s in PASS_F64] + [("f32",) + s for s in PASS_F32]


def _pass_inputs(m, n, dtype):
    T = _types(dtype)[0]
    rng = np.random.default_rng(7 * m + n)
    A = (rng.standard_normal((m, n)) / math.sqrt(n)).astype(T)
    x = (rng.standard_normal(n) * rng.choice([0, 3e-4, 1e-3, 3e-2, 1.0], n)).astype(T)
    x[0] = T(0.3 * THRES)
    x[n - 1] = T(0.7)
    xt, _ = thr_T(x, THRES)
    b = rng.standard_normal(m).astype(T)
    return A, x, xt, b


def _expected_blocks(m):
    return max(1, min(256, (m + 7) // 8))


@pytest.mark.parametrize("dtype,m,n", PASS_CASES)
def test_descent_pass(dtype, m, n):
    A, x, xt, b = _pass_inputs(m, n, dtype)
    assert not _same_bits(x, xt)
    Ad, xd, xtd, bd = _dev(A), _dev(x), _dev(xt), _dev(b)
    rn = torch.tensor([1.7320508], dtype=torch.float64, device=DEV)
    k = _k()
    o = _out_np(k.descent_pass(Ad, xd, xtd, bd, fh_mu=FH_MU, rn=rn))
    blocks = o["blocks"]
    assert blocks == _expected_blocks(m)
    ref = ref_pass(A, x, xt, b, blocks)
    assert ref["sums"][0] != ref["sums"][1]
    _check_close("G (pass)", dtype, o["G"], ref["G"], ref["BG"])
    for i in (0, 1):
        _check_sum("sum r%d^2" % (i + 1), dtype, o["sums"][i], ref["sums"][i], ref["sbnd"][i])
    assert o["fh"][0] == 0.5 * float(o["sums"][0]) + FH_MU * 1.7320508, "fh"
    # the same bits from both read policies of A, without the record, and on a second run
    for nt, kw in ((0, {}), (1, {}), (-1, dict(fh_mu=FH_MU, rn=rn))):
        o2 = _out_np(k.descent_pass(Ad, xd, xtd, bd, nt=nt, **kw))
        assert _same_bits(o["G"], o2["G"]) and _same_bits(o["sums"], o2["sums"]), nt
        assert (o2["fh"] is None) if not kw else _same_bits(o["fh"], o2["fh"])


@pytest.mark.parametrize("dtype,n", [("f64", 1031), ("f64", 8194), ("f32", 16388)])
def test_descent_pass_refuses(dtype, n):
    from glx import _lib
    m = 9
    A, x, xt, b = _pass_inputs(m, n, dtype)
    G = torch.full((n,), -3.0, dtype=torch.float64 if dtype == "f64" else torch.float32, device=DEV)
    sums = torch.full((2,), -5.0, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.GlxError) as ei:
        _k().descent_pass(_dev(A), _dev(x), _dev(xt), _dev(b), G=G, sums=sums)
    assert ei.value.code == 1 and str(n) in str(ei.value)      # GLX_E_INVALID, with a message
    assert bool((G == -3.0).all()) and bool((sums == -5.0).all())
