"""An unpenalised intercept on the GPU (DESIGN.md "Intercept"). Reference: tests/ic_ref.py, which forms
the centred pair (P~ A~, P~ b~) explicitly and applies the existing references to it; the library never
forms it.

1. The centring finalize (glx.kernels.cert_fin_ic, two launches). r^ = fl(sum of the slabs in slab
   order) - b is one rounded operation per element on values the test holds exactly: bit for bit against
   NumPy in the dtype. A mean sums m products w r^ (one rounding each) with m - 1 additions in some fixed
   order and one division: gamma_{m+2}(eps64) sum w |r^| / sigma against longdouble. r_c = (T)((double) r^
   - mean) and r_w = fl(w r_c) are reproduced from the DEVICE's means, bit for bit. The three sums are
   k_cert_fin_w's on r_c: gamma_{ml+3}(eps64) sum |terms| against longdouble on the same r_c.
2. The centred column norms (glx.kernels.col_norms_ic). A term is (w d) d with d = fl(a - mean) in double:
   four roundings, then m - 1 additions and a root: the stored norm is low by at most gamma_{m+5}(eps64)
   relative (the guard's own bar), and high by at most that plus sqrt(sigma) |mean^ - mean| <=
   gamma_{m+2}(eps64) ||a~_i|| (any mean but the exact one only enlarges sum w (a - mean)^2).
3. Certificates against ic_ref with test_gpu_sample_weight's bars, the centring carried through them:
   d(mean) = w^T dr / sigma + (m + 2) eps64 w^T |r| / sigma, dr_c = dr + d(mean) + eps |r_c|,
   d(w r_c) = w dr_c + eps / 2 |w r_c|, dg = (m + 2) eps |A|^T |w r_c| + |A|^T d(w r_c).
4. Solves: test_gpu_sample_weight.test_general_weights_solve's assertions with gap+ from ic_ref.guard on the
   solve's own record.
"""
import functools
import io

import numpy as np
import pytest

import group_ref as gr
import ic_ref as ic
import screen_ref as sr
import sw_ref as sw

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS64 = sr.EPS64


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(a, dtype=None):
    torch = _torch()
    a = np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a).astype(dtype)
    return torch.as_tensor(a, device="cuda")


def _eps(dt):
    return float(np.finfo(dt).eps)


def _np(t):
    return None if t is None else t.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1
def _fin_weights(g, m, dt):
    w = g.uniform(0.0, 3.0, m).astype(dt)
    w[::4] = 0
    if m > 1:
        w[1] = 1.25                                # (row 0 weighs 0: sigma stays positive at every m)
    v = g.uniform(0.0, 2.0, m).astype(dt)
    v[1::3] = 0
    return w, v


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("S", [0, 1, 3])
# (one block; ragged l; l = 1; 2050 x 128 and 262147 x 1: 1025 row groups, past the column-sum kernel's
# cap of 256 workgroups and past the centred finalize's of 1024)
@pytest.mark.parametrize("shape", [(5, 3), (64, 16), (67, 1), (130, 128), (2050, 128), (262147, 1)],
                         ids=lambda s: "%dx%d" % s)
def test_centring_finalize(shape, S, dt):
    from glx import kernels
    m, l = shape
    g = np.random.default_rng(1000 * m + 10 * l + S)
    b = (g.standard_normal((m, l)) + 3.0 * g.standard_normal(l)[None, :]).astype(dt)
    P = g.standard_normal((S, m, l)).astype(dt) if S else None
    w, v = _fin_weights(g, m, dt)
    sigma = float(np.sum(w, dtype=np.float64))
    ax = np.zeros((m, l), dtype=dt)
    if S:
        ax = P[0].copy()
        for k in range(1, S):
            ax = (ax + P[k]).astype(dt)
    rh = (ax - b).astype(dt)
    Pd = None if P is None else _dev(P)
    out = kernels.cert_fin_ic(Pd, _dev(b), _dev(w), _dev(v))
    got = {k: _np(t) for k, t in out.items()}
    # the column-sum finalize
    assert np.array_equal(got["rhat"], rh)
    wl, rl, bl = w.astype(LD)[:, None], rh.astype(LD), b.astype(LD)
    mean_ref = np.sum(wl * rl, axis=0) / LD(sigma)
    mean_bar = sr.gamma(m + 2, EPS64) * np.sum(wl * np.abs(rl), axis=0).astype(np.float64) / sigma
    merr = np.abs((got["means"].astype(LD) - mean_ref).astype(np.float64))
    print("csum %s S=%d %s: worst mean err / bar %.3f" % (shape, S, dt.__name__,
                                                          float(np.max(merr / np.maximum(mean_bar, 1e-300)))))
    assert np.all(merr <= mean_bar)
    # the centred finalize, from the device's own means
    rc = (rh.astype(np.float64) - got["means"][None, :]).astype(dt)
    with np.errstate(under="ignore"):
        rw = (w[:, None] * rc).astype(dt)
    assert np.array_equal(got["rc"], rc) and np.array_equal(got["rw"], rw)
    cl = rc.astype(LD)
    terms = [wl * cl * cl, wl * cl * bl, v.astype(LD)[:, None] * cl * cl]
    gam = sr.gamma(m * l + 3, EPS64)
    for i, t in enumerate(terms):
        err, bar = abs(float(LD(got["sums"][i]) - np.sum(t))), gam * float(np.sum(np.abs(t)))
        print("fin_c %s S=%d %s sum %d: err %.3e bar %.3e" % (shape, S, dt.__name__, i, err, bar))
        assert err <= bar, (i, err, bar)
    again = kernels.cert_fin_ic(Pd, _dev(b), _dev(w), _dev(v))
    for key in ("rhat", "means", "rc", "rw", "sums"):
        assert np.array_equal(_np(again[key]), got[key]), key
    # without hold-out weights: the same two sums, the third slot untouched; r_c not asked for
    two = kernels.cert_fin_ic(Pd, _dev(b), _dev(w), None, want_rc=False)
    s2 = _np(two["sums"])
    assert two["rc"] is None and np.array_equal(s2[:2], got["sums"][:2]) and np.isnan(s2[2])
    assert np.array_equal(_np(two["rw"]), rw) and np.array_equal(_np(two["means"]), got["means"])
    # all-ones weights give the bits of the null-weight form
    one = kernels.cert_fin_ic(Pd, _dev(b), _dev(np.ones(m, dtype=dt)), None)
    none = kernels.cert_fin_ic(Pd, _dev(b), None, None)
    for key in ("rhat", "means", "rc", "rw"):
        assert np.array_equal(_np(one[key]), _np(none[key])), key
    assert np.array_equal(_np(one["sums"])[:2], _np(none["sums"])[:2])
    assert np.array_equal(_np(none["rw"]), _np(none["rc"]))


def test_centring_finalize_nan_reaches_the_sums():
    from glx import kernels
    m, l = 67, 5
    g = np.random.default_rng(9)
    b = g.standard_normal((m, l))
    P = g.standard_normal((1, m, l))
    P[0, 40, 2] = np.nan
    w = g.uniform(0.5, 2.0, m)
    out = kernels.cert_fin_ic(_dev(P), _dev(b), _dev(w), _dev(w))
    means, sums = _np(out["means"]), _np(out["sums"])
    assert np.isnan(means[2]) and not np.any(np.isnan(np.delete(means, 2)))
    assert np.all(np.isnan(sums))
    assert np.all(np.isnan(_np(out["rc"])[:, 2])) and not np.any(np.isnan(np.delete(_np(out["rc"]), 2, axis=1)))


# ------------------------------------------------------------------------------------------ 2
def _chunked(fn, A, w, step=16384):
    return np.concatenate([fn(A[:, j:j + step], w) for j in range(0, A.shape[1], step)])


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
# (test_gpu_sample_weight.test_weighted_col_norms' shapes: m x 262214 is 70 columns past the cap of 1024
# column blocks, in one slab and in three)
@pytest.mark.parametrize("shape", [(1, 1), (63, 65), (130, 300), (4097, 70), (3, 262214), (130, 262214)],
                         ids=lambda s: "%dx%d" % s)
def test_centred_col_norms(shape, dt):
    from glx import kernels
    m, n = shape
    g = np.random.default_rng(31 * m + n)
    A = (g.standard_normal((m, n)) + g.standard_normal(n)[None, :]).astype(dt)
    w = g.uniform(0.0, 3.0, m).astype(dt)
    if m > 1:
        w[::3] = 0                                  # a zero-weight row set
    else:
        w[:] = 1.5
    const_col, wconst_col = n // 2, n // 3
    A[:, const_col] = dt(2.5)                       # constant everywhere
    if n > 2:
        A[w != 0, wconst_col] = dt(-1.75)           # constant on the weighted rows only
    sigma = float(np.sum(w, dtype=np.float64))
    want = _chunked(ic.col_norms, A, w)
    mean_ref = _chunked(ic.col_means, A, w)
    un = _chunked(sw.col_norms, A, w).astype(np.float64)
    Ad = _dev(A)
    norms, means, stats = kernels.col_norms_ic(Ad, _dev(w))
    got, gm, st = _np(norms), _np(means), _np(stats)
    wabs = (w.astype(np.float64) @ np.abs(A.astype(np.float64))) / sigma
    assert np.all(np.abs((gm.astype(LD) - mean_ref).astype(np.float64)) <= sr.gamma(m + 2, EPS64) * wabs)
    # (the reference's own error: longdouble means and differences, relative to the uncentred scale)
    ref_err = (m + 5) * float(np.finfo(LD).eps) * un
    low = sr.gamma(m + 5, EPS64) * want.astype(np.float64) + ref_err
    high = low + sr.gamma(m + 2, EPS64) * un
    diff = (got.astype(LD) - want).astype(np.float64)
    print("centred norms %s %s: worst below / bar %.3f, above / bar %.3f"
          % (shape, dt.__name__, float(np.max(-diff / np.maximum(low, 1e-300))),
             float(np.max(diff / np.maximum(high, 1e-300)))))
    assert np.all(diff >= -low) and np.all(diff <= high)
    assert got[const_col] <= sr.gamma(m + 2, EPS64) * un[const_col]          # 0 or rounding dust
    assert got[wconst_col] <= sr.gamma(m + 2, EPS64) * un[wconst_col]
    assert st[0] == got.max() and st[2] == np.abs(gm).max()
    sq, sa = float(np.sum(got.astype(LD) ** 2)), float(np.sum(gm.astype(LD) ** 2))
    assert abs(st[1] - sq) <= (m + n + 2) * EPS64 * sq and abs(st[3] - sa) <= (n + 2) * EPS64 * sa
    n2, m2, s2 = kernels.col_norms_ic(Ad, _dev(w))
    assert np.array_equal(_np(n2), got) and np.array_equal(_np(m2), gm) and np.array_equal(_np(s2), st)
    a1, b1, c1 = kernels.col_norms_ic(Ad, _dev(np.ones(m, dtype=dt)))
    a0, b0, c0 = kernels.col_norms_ic(Ad, None)
    assert np.array_equal(_np(a1), _np(a0)) and np.array_equal(_np(b1), _np(b0)) and np.array_equal(_np(c1), _np(c0))


def test_centred_col_norms_nan_weight_reaches_the_maximum():
    from glx import kernels
    A = np.arange(5 * 70, dtype=np.float64).reshape(5, 70)
    w = np.ones(5)
    w[3] = np.nan
    norms, means, stats = kernels.col_norms_ic(_dev(A), _dev(w), sigma=4.0)
    assert np.all(np.isnan(_np(norms))) and np.isnan(_np(stats)[0]) and np.isnan(_np(stats)[2])


# ------------------------------------------------------------------------------------------ 3
CERT_SHAPES = [(96, 512, 16), (40, 130, 3)]


def _groups_for(n, seed=5):
    ptr = gr.draw_groups(np.random.default_rng(seed), n, sw.GROUP_SIZES)
    return ptr, np.sqrt(np.diff(ptr).astype(np.float64))


def _icert_bars(x, A, b, mu, w, dt, zero_x=False):
    """test_gpu_sample_weight._wcert_bars with the centring carried through (docstring, 3). Also returns
    the bar of the intercept."""
    import test_gpu_certificate as tc
    W = tc._wide(dt)
    eps = _eps(dt)
    m, n = A.shape
    muT = float(dt(mu))
    ref = ic.certificate(x, A, b, muT, w, wide=W)
    A64, x64, b64 = (np.abs(a.astype(np.float64)) for a in (A, x, b))
    w64 = w.astype(np.float64)[:, None]
    sigma = float(np.sum(w64))
    r = A.astype(W) @ x.astype(W) - b.astype(W)
    rc_true = np.abs((r - (w.astype(W) @ r)[None, :] / W(sigma)).astype(np.float64))
    r_abs = np.abs(r.astype(np.float64))
    dr = np.zeros(b.shape) if zero_x else (n + 2) * eps * (A64 @ x64 + b64)
    dmean = np.sum(w64 * dr, axis=0) / sigma + (m + 2) * EPS64 * np.sum(w64 * r_abs, axis=0) / sigma
    drc = dr + dmean[None, :] + eps * rc_true
    drw = w64 * drc + eps / 2 * w64 * rc_true
    dg = (m + 2) * eps * (A64.T @ (w64 * rc_true)) + A64.T @ drw
    g_T = ref["g"].astype(dt)
    _, bars = tc._row_bars(x, g_T, muT, dt, dg=dg + eps / 2 * np.abs(ref["g"].astype(np.float64)))
    rr, rb = float(ref["rr"]), float(ref["rb"])
    bars["rr"] = tc.C * (np.sum(w64 * (2 * rc_true * drc + drc * drc)) + (tc.CSUM + 2) * EPS64 * rr)
    bars["rb"] = tc.C * (np.sum(w64 * b64 * drc) + (tc.CSUM + 2) * EPS64 * np.sum(w64 * rc_true * b64))
    gmax, s, sx = float(ref["gmax"]), float(ref["scale"]), float(ref["sum_xnorm"])
    dgm = bars["gmax"] / tc.C
    ds = min(1.0, muT / max(gmax - dgm, tc.TINY)) - min(1.0, muT / (gmax + dgm)) if gmax > 0 else 0.0
    host = 4 * EPS64 * (0.5 * (1 + s * s) * rr + abs(s * rb) + muT * sx)
    bars["gap"] = tc.C * (0.5 * (1 + s * s) * bars["rr"] / tc.C + s * bars["rb"] / tc.C
                          + muT * bars["sum_xnorm"] / tc.C + abs(s * rr + rb) * ds + host)
    bars["intercept"] = tc.C * dmean
    return ref, bars


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["ones", "general"])
@pytest.mark.parametrize("shape", CERT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_certificate_with_an_intercept(shape, kind, dt):
    import glx
    m, n, l = shape
    A, b = ic.offset_instance(m, n, l)
    A, b = A.astype(dt), b.astype(dt)
    w = sw.weights_of(kind, m).astype(dt)
    sw_arg = None if kind == "ones" else w
    W = np.longdouble if dt == np.float64 else np.float64
    # mu_max is the certificate's gmax at x = 0, and there the intercept is b-bar
    want = float(ic.mu_max(A, b, w, wide=W))
    mm = glx.mu_max(A, b, sample_weight=sw_arg, fit_intercept=True)
    zero = np.zeros((n, l), dtype=dt)
    _, bars0 = _icert_bars(zero, A, b, want, w, dt, zero_x=True)
    print("mu_max %s %s %s: got %.17g ref %.17g bar %.3e" % (shape, kind, dt.__name__, mm, want, bars0["gmax"]))
    assert abs(mm - want) <= bars0["gmax"]
    c0 = glx.certificate(zero, A, b, mm, sample_weight=sw_arg, fit_intercept=True)
    ref0, bars0 = _icert_bars(zero, A, b, mm, w, dt, zero_x=True)
    assert c0["gmax"] == mm and c0["scale"] == 1.0 and c0["kkt_max"] == 0.0 and c0["nonzero_rows"] == 0
    assert abs(c0["gap"]) <= bars0["gap"]
    bbar = (w.astype(W) @ b.astype(W)) / np.sum(w.astype(W))
    assert np.all(np.abs(c0["intercept"] - bbar.astype(np.float64)) <= bars0["intercept"] + 2 * EPS64 * np.abs(bbar))
    assert mm < 0.9 * glx.mu_max(A, b, sample_weight=sw_arg)          # (the offsets: another problem)
    # a random sparse point
    g = np.random.default_rng(12)
    x = (g.standard_normal((n, l)) * (g.random((n, 1)) < 0.2) * 0.05).astype(dt)
    mu = float(dt(0.3 * want))
    ref, bars = _icert_bars(x, A, b, mu, w, dt)
    c = glx.certificate(x, A, b, mu, sample_weight=sw_arg, row_norms=True, fit_intercept=True)
    assert "k_cert_csum" in c["plan"] and "k_cert_fin_c" in c["plan"]
    for key in ("gmax", "kkt_max", "gap"):
        err = abs(float(c[key]) - float(ref[key]))
        print("intercept certificate %s %s %s %s: err %.3e bar %.3e" % (shape, kind, dt.__name__, key, err, bars[key]))
        assert err <= bars[key], (key, err, bars[key])
    perr = abs(c["primal"] - float(ref["primal"]))
    assert perr <= 0.5 * bars["rr"] + mu * bars["sum_xnorm"] + 4 * EPS64 * abs(float(ref["primal"]))
    assert np.all(np.abs(c["row_norms"] - ref["row_norms"].astype(np.float64)) <= bars["gnorm"])
    assert c["nonzero_rows"] == ref["nonzero_rows"]
    ierr = np.abs(c["intercept"] - ref["intercept"].astype(np.float64))
    print("intercept %s %s %s: worst err / bar %.3f" % (shape, kind, dt.__name__,
                                                        float(np.max(ierr / bars["intercept"]))))
    assert c["intercept"].dtype == np.float64 and c["intercept"].shape == (l,)
    assert np.all(ierr <= bars["intercept"] + 2 * EPS64 * np.abs(ref["intercept"].astype(np.float64)))
    if kind == "ones":      # all-ones weights: the bits of the call without weights
        c1 = glx.certificate(x, A, b, mu, sample_weight=w, row_norms=True, fit_intercept=True)
        for key in ("primal", "dual", "gap", "gmax", "kkt_max", "kkt_fro", "nonzero_rows"):
            assert c[key] == c1[key], key
        assert np.array_equal(c["intercept"], c1["intercept"]) and np.array_equal(c["row_norms"], c1["row_norms"])
    # groups on top: the loss terms are the row certificate's (the same finalize), gmax within the group bar
    ptr, gw = _groups_for(n)
    cg = glx.certificate(x, A, b, mu, groups=ptr, weights=gw, sample_weight=sw_arg, fit_intercept=True)
    refg = ic.certificate(x, A, b, mu, w, ptr, gw, wide=W)
    K = int(np.diff(ptr).max()) * l
    gK = sr.gamma(K + 3, _eps(dt))
    dgq = np.sqrt(np.add.reduceat(bars["gnorm"] ** 2, ptr[:-1].astype(np.intp))) / gw
    bar_g = float(np.max(dgq)) + 2 * gK * float(refg["gmax"])
    assert abs(cg["gmax"] - float(refg["gmax"])) <= bar_g, (cg["gmax"], float(refg["gmax"]), bar_g)
    assert np.array_equal(cg["intercept"], c["intercept"]) and cg["nonzero_groups"] == refg["nonzero_groups"]
    assert "k_cert_csum" in cg["plan"]


# ------------------------------------------------------------------------------------------ 4
SOLVE_CASES = [(m, n, l, ratio, kind) for (m, n, l) in CERT_SHAPES for kind in ("ones", "general")
               for ratio in (0.5, 0.1)]
TOL = 1e-10


def _record_ic(x, A, b, mu, w, gw=None):
    from glx.certificate import _inputs, _record_ic as rec_ic, _sigma, _sw_device
    xd, Ad, bd = _inputs(x, A, b)
    wa = np.ascontiguousarray(w, dtype=A.dtype)
    rec, _, _, _, icpt = rec_ic(xd, Ad, bd, mu, 0, False, _sw_device(wa, Ad.device), _sigma(wa, A.shape[0]), None, gw)
    return rec, icpt


def _gap_plus(x, A, b, mu, w, eps=EPS64):
    """gap+ of the intercept guard from the GPU's own record of x."""
    m, n = A.shape
    rec, icpt = _record_ic(x, A, b, mu, w)
    cst, bn, sigma = ic.figures(A, b, w)
    return ic.guard(rec, mu, eps, m, n, b.shape[1], cst, bn, sigma, float(np.sum(icpt * icpt)))[1]


@functools.lru_cache(maxsize=None)
def _solved(m, n, l, ratio, kind, f32=False, tol=TOL):
    import glx
    ref = ic.reference_solution(m, n, l, ratio, kind, f32)
    dt = np.float32 if f32 else np.float64
    return glx.solve_certified(ref["A"].astype(dt), ref["b"].astype(dt), ref["mu"], tol=tol,
                               sample_weight=None if kind == "ones" else ref["w"], fit_intercept=True)


@pytest.mark.parametrize("case", SOLVE_CASES, ids=lambda c: "%dx%dx%d@%g-%s" % c)
def test_intercept_solve(case):
    m, n, l, ratio, kind = case
    ref = ic.reference_solution(m, n, l, ratio, kind)
    A, b, w, mu = ref["A"].copy(), ref["b"].copy(), ref["w"].copy(), ref["mu"]
    x, info = _solved(m, n, l, ratio, kind)
    assert info["converged"] and info["rel_gap"] <= TOL
    gp = _gap_plus(x, A, b, mu, w)
    c = info["intercept"]
    excess = float(ic.primal(x, c, A, b, mu, w) - ic.primal(ref["x"], ref["c"], A, b, mu, w))
    print("intercept %s: P(x, c) - P* %.3e, reported gap %.3e, gap+ %.3e, %d iterations, compactions %s, kept %d"
          % (case, excess, info["gap"], gp, info["iterations"], info["kept_history"], info["kept"]))
    assert excess <= gp and gp <= info["gap"] + 10 * TOL * info["primal"]
    assert excess >= -float(ref["gap"]) - 4 * EPS64 * info["primal"]
    support = np.nonzero(np.sqrt(np.sum(ref["x"] ** 2, axis=1)) != 0)[0]
    assert set(support) <= set(info["kept_rows"].tolist())
    screened = np.ones(n, dtype=bool)
    screened[info["kept_rows"]] = False
    assert not np.any(screened & ~(ref["gtheta"] < LD(mu)))
    if ratio == 0.5:
        assert info["compactions"] >= 1 and info["width"] < n
    assert "k_cert_csum" in info["plan"] and "k_cert_fin_c" in info["plan"]
    # the intercept is c(x) of the returned x
    cx = ic.intercept_of(x, A, b, w).astype(np.float64)
    assert c.dtype == np.float64 and c.shape == (l,)
    assert np.all(np.abs(c - cx) <= 1e-12 * (np.abs(cx) + 1.0))


def test_intercept_grouped_solve():
    import glx
    m, n, l, ratio = 96, 512, 16, 0.5
    ref = ic.group_reference_solution(m, n, l, ratio)
    A, b, w, ptr, gw, mu = (ref[k].copy() if hasattr(ref[k], "copy") else ref[k]
                            for k in ("A", "b", "w", "ptr", "gw", "mu"))
    x, info = glx.solve_certified(A, b, mu, tol=TOL, groups=ptr, weights=gw, sample_weight=w, fit_intercept=True)
    assert info["converged"] and info["compactions"] >= 1
    Ac, _ = ic.centre(A, b, w)
    gcn = np.asarray(gr.group_cnorms(Ac, ptr, gw), dtype=np.float64)
    rec, icpt = _record_ic(x, A, b, mu, w, (np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(gw)))
    cst, bn, sigma = ic.figures(A, b, w)
    gp = ic.group_guard(rec, mu, EPS64, m, n, l, int(np.diff(ptr).max()), float(gw.min()), float(gcn.max()), cst, bn,
                        sigma, float(np.sum(icpt * icpt)))[1]
    excess = float(ic.primal(x, info["intercept"], A, b, mu, w, ptr, gw)
                   - ic.primal(ref["x"], ref["c"], A, b, mu, w, ptr, gw))
    print("grouped: P(x, c) - P* %.3e gap+ %.3e reported %.3e, kept %d groups"
          % (excess, gp, info["gap"], info["kept"]))
    assert excess <= gp
    active = np.nonzero(gr.group_norms(ref["x"], ptr) != 0)[0]
    assert set(active) <= set(info["kept_groups"].tolist())
    assert "k_cert_csum" in info["plan"]


def test_intercept_solve_f32():
    m, n, l, ratio = 96, 512, 16, 0.5
    ref = ic.reference_solution(m, n, l, ratio, "general", True)
    x, info = _solved(m, n, l, ratio, "general", True, 1e-4)
    print("f32: %d iterations, compactions %s, kept %d, rel_gap %.2e"
          % (info["iterations"], info["kept_history"], info["kept"], info["rel_gap"]))
    assert x.dtype == np.float32 and info["converged"]
    screened = np.ones(n, dtype=bool)
    screened[info["kept_rows"]] = False
    assert not np.any(screened & ~(ref["gtheta"] < LD(ref["mu"])))
    assert not np.any(screened & (np.sqrt(np.sum(ref["x"] ** 2, axis=1)) != 0))


# ------------------------------------------------------------------------------------------ an equal problem
@pytest.mark.parametrize("case", [(40, 130, 3, 0.1, "general"), (96, 512, 16, 0.5, "ones")],
                         ids=lambda c: "%dx%dx%d@%g-%s" % c)
def test_the_explicitly_centred_problem_has_the_same_solution(case):
    """solve_certified on explicitly centred fp64 copies (no intercept) solves the same problem: the two
    solutions are within sqrt(2 g1) + sqrt(2 g2) in the centred seminorm ||P~ A~ (x1 - x2)||."""
    import glx
    from glx.certificate import record
    m, n, l, ratio, kind = case
    ref = ic.reference_solution(m, n, l, ratio, kind)
    A, b, w, mu = ref["A"].copy(), ref["b"].copy(), ref["w"].copy(), ref["mu"]
    x1, i1 = _solved(m, n, l, ratio, kind)
    Ac, bc = ic.centre(A, b, w)
    Ac, bc = np.ascontiguousarray(Ac), np.ascontiguousarray(bc)
    x2, i2 = glx.solve_certified(Ac, bc, mu, tol=TOL)
    assert i1["converged"] and i2["converged"]
    g1 = _gap_plus(x1, A, b, mu, w)
    cn = np.asarray(sr.col_norms(Ac), dtype=np.float64)
    g2 = sr.guard(record(x2, Ac, bc, mu), mu, EPS64, m, n, l, float(cn.max()), float(np.sum(cn * cn)),
                  float(np.sqrt(np.sum(bc * bc))))[1]
    d = Ac.astype(LD) @ (x1 - x2).astype(LD)
    dist, bound = float(np.sqrt(np.sum(d * d))), np.sqrt(2 * g1) + np.sqrt(2 * g2)
    P1, P2 = ic.primal(x1, i1["intercept"], A, b, mu, w), ic.primal(x2, ic.intercept_of(x2, A, b, w), A, b, mu, w)
    print("equal problem %s: ||P~ A~ (x1 - x2)|| %.3e bound %.3e; |P1 - P2| %.3e bound %.3e"
          % (case, dist, bound, float(abs(P1 - P2)), g1 + g2))
    assert dist <= bound and float(abs(P1 - P2)) <= g1 + g2
    assert g1 <= 10 * TOL * float(P1) and g2 <= 10 * TOL * float(P1)


# ------------------------------------------------------------------------------------------ invariances
def test_a_constant_added_to_b_moves_only_the_intercept():
    import glx
    m, n, l, ratio, kind = 40, 130, 3, 0.1, "general"
    ref = ic.reference_solution(m, n, l, ratio, kind)
    A, b, w, mu = ref["A"].copy(), ref["b"].copy(), ref["w"].copy(), ref["mu"]
    d = np.array([2.0, -1.0, 0.5])
    x1, i1 = _solved(m, n, l, ratio, kind)
    b2 = b + d[None, :]
    x2, i2 = glx.solve_certified(A, b2, mu, tol=TOL, sample_weight=w, fit_intercept=True)
    assert i2["converged"]
    g1, g2 = _gap_plus(x1, A, b, mu, w), _gap_plus(x2, A, b2, mu, w)
    # each intercept is c(x) of its own x on its own b, so their difference is d up to a-bar^T (x1 - x2)
    abar = ic.col_means(A, w)
    shift = (i2["intercept"] - i1["intercept"] - d).astype(LD) + abar @ (x2 - x1).astype(LD)
    assert np.all(np.abs(shift.astype(np.float64)) <= 1e-12 * (np.abs(d) + np.abs(i1["intercept"]) + 1.0))
    P1 = float(ic.primal(x1, i1["intercept"], A, b, mu, w))
    P2 = float(ic.primal(x2, i2["intercept"], A, b2, mu, w))
    print("shifted b: intercepts %s -> %s, |P1 - P2| %.3e, gap+ %.3e %.3e, kept %d / %d"
          % (i1["intercept"], i2["intercept"], abs(P1 - P2), g1, g2, i1["kept"], i2["kept"]))
    assert abs(P1 - P2) <= g1 + g2 and abs(i1["primal"] - i2["primal"]) <= g1 + g2 + 8 * EPS64 * P1
    assert np.array_equal(i1["kept_rows"], i2["kept_rows"])
    assert np.max(np.abs(i2["intercept"] - i1["intercept"] - d)) < 1e-3       # (and it did move by d)


def test_fit_intercept_false_is_the_call_without_the_keyword():
    import glx
    m, n, l = 40, 130, 3
    A, b = ic.offset_instance(m, n, l)
    w = sw.weights_of("general", m)
    mu = 0.3 * glx.mu_max(A, b, sample_weight=w)
    assert glx.mu_max(A, b, sample_weight=w, fit_intercept=False) == glx.mu_max(A, b, sample_weight=w)
    for kw in ({}, {"sample_weight": w}):
        xa, ia = glx.solve_certified(A, b, mu, tol=1e-8, **kw)
        xb, ib = glx.solve_certified(A, b, mu, tol=1e-8, fit_intercept=False, **kw)
        assert np.array_equal(xa, xb) and set(ia) == set(ib) and "intercept" not in ib
        for key in ia:
            if key == "tt":
                continue
            same = np.array_equal(ia[key], ib[key]) if isinstance(ia[key], np.ndarray) else ia[key] == ib[key]
            assert same, key
        x0 = np.asarray(xa)
        ca, cb = glx.certificate(x0, A, b, mu, **kw), glx.certificate(x0, A, b, mu, fit_intercept=False, **kw)
        assert ca == cb and "intercept" not in cb
    pa = glx.path(A, b, n_mus=3, mu_min_ratio=0.1, tol=1e-6)
    pb = glx.path(A, b, n_mus=3, mu_min_ratio=0.1, tol=1e-6, fit_intercept=False)
    for (m1, x1, i1), (m2, x2, i2) in zip(pa, pb):
        assert m1 == m2 and np.array_equal(x1, x2) and i1["plan"] == i2["plan"] and i1["gap"] == i2["gap"]


# ------------------------------------------------------------------------------------------ hold-out, path, CV
def _holdout_bar(x, c, A, b, v, eps):
    """test_gpu_sample_weight._holdout_bar for r_c = fl(r^ + c) with the returned c: the product's bar and
    the centring's one rounding carried through v, plus the fp64 sum's."""
    m, n = A.shape
    l = b.shape[1]
    r = np.abs(A.astype(LD) @ x.astype(LD) + c.astype(LD)[None, :] - b.astype(LD)).astype(np.float64)
    an = np.sqrt(np.sum(A.astype(np.float64) ** 2, axis=1))[:, None]
    xn = np.sqrt(np.sum(x.astype(np.float64) ** 2, axis=0))[None, :]
    dr = sr.gamma(n + 2, eps) * an * xn + eps * (r + np.abs(b.astype(np.float64))) + eps * r
    vv = v.astype(np.float64)[:, None]
    total = float(np.sum(vv * r * r))
    bar_sum = float(np.sum(vv * (2 * r * dr + dr * dr))) + sr.gamma(m * l + 3, EPS64) * total
    return 0.5 * bar_sum / float(np.sum(v)) + 4 * EPS64 * 0.5 * total / float(np.sum(v))


def test_holdout_loss_uses_the_training_intercept():
    import glx
    m, n, l = 40, 130, 3
    A, b = ic.offset_instance(m, n, l)
    lab = np.arange(m) % 4
    tr, ho = (lab != 1).astype(np.float64) * 1.5, (lab == 1).astype(np.float64) * 0.5
    mu = 0.1 * glx.mu_max(A, b, sample_weight=tr, fit_intercept=True)
    x, info = glx.solve_certified(A, b, mu, tol=1e-8, sample_weight=tr, holdout_weight=ho, fit_intercept=True)
    c = info["intercept"]
    want = float(ic.holdout_loss(x, c, A, b, ho))
    bar = _holdout_bar(x, c, A, b, ho, EPS64)
    print("holdout_loss: got %.17g ref %.17g err %.3e bar %.3e" % (info["holdout_loss"], want,
                                                                   abs(info["holdout_loss"] - want), bar))
    assert info["converged"] and abs(info["holdout_loss"] - want) <= bar
    assert info["holdout_loss"] == 0.5 * info["holdout_sum"] / float(np.sum(ho))
    assert abs(float(sw.holdout_loss(x, A, b, ho)) - want) > 100 * bar       # (without the intercept: another number)
    # hold-out weights alone: held out of the unweighted fit
    x2, i2 = glx.solve_certified(A, b, mu, tol=1e-8, holdout_weight=ho, fit_intercept=True)
    x3, i3 = glx.solve_certified(A, b, mu, tol=1e-8, sample_weight=np.ones(m), holdout_weight=ho, fit_intercept=True)
    assert np.array_equal(x2, x3) and i2["holdout_loss"] == i3["holdout_loss"]


def test_path_with_an_intercept():
    import glx
    m, n, l = 96, 512, 16
    A, b = ic.offset_instance(m, n, l)
    w = sw.weights_of("general", m)
    tol = 1e-6
    out = glx.path(A, b, n_mus=4, mu_min_ratio=0.05, tol=tol, sample_weight=w, fit_intercept=True)
    mus = [o[0] for o in out]
    assert mus[0] == glx.mu_max(A, b, sample_weight=w, fit_intercept=True) and len(out) == 4
    mu0, x0, i0 = out[0]
    bbar = ((w.astype(LD) @ b.astype(LD)) / np.sum(w.astype(LD))).astype(np.float64)
    assert np.all(x0 == 0) and i0["iterations"] == 0 and i0["converged"] and abs(i0["gap"]) <= 1e-12 * i0["primal"]
    assert np.all(np.abs(i0["intercept"] - bbar) <= 1e-13 * (np.abs(bbar) + 1.0))
    for mu, x, info in out:
        assert info["converged"] and info["rel_gap"] <= tol and info["mu"] == mu and info["intercept"].shape == (l,)
    warm = sum(o[2]["iterations"] for o in out)
    cold = sum(glx.solve_certified(A, b, mu, tol=tol, sample_weight=w, fit_intercept=True)[1]["iterations"]
               for mu in mus)
    print("intercept path: warm-started %d iterations, cold %d" % (warm, cold))
    assert warm < cold


def test_cv_path_with_an_intercept():
    """The cross-validation instance with the offsets, K = 5, ten mu. The reference curve (ic_ref.cv_reference,
    re-derived on the CPU in test_intercept_cpu.test_cv_reference_indices_with_an_intercept at 1e-6 and
    here checked at 1e-8 too when it was written): best = 5, one_se = 5; the runner-up mean is 5.2 % above
    the minimum, mean[4] is 0.77 % above the 1-SE threshold, and the two tolerances move a mean by at
    most 3.5e-5 relative."""
    import glx
    A, b = ic.cv_instance()
    cv = glx.cv_path(A, b, folds=5, n_mus=10, mu_min_ratio=1e-2, tol=1e-6, fit_intercept=True)
    assert cv["folds"] == 5 and cv["fold_loss"].shape == (5, 10) and len(cv["mus"]) == 10
    assert cv["mus"][0] == glx.mu_max(A, b, fit_intercept=True)
    print("cv mean %s\ncv se %s\nbest %d one_se %d" % (np.round(cv["mean"], 4), np.round(cv["se"], 4), cv["best"],
                                                       cv["one_se"]))
    assert cv["best"] == 5 and cv["one_se"] == 5
    mean, se, best, one = sw.cv_aggregate(cv["fold_loss"])
    assert (best, one) == (5, 5)
    for k in range(5):
        assert len(cv["info"][k]) == 10 and all(i["converged"] and i["intercept"].shape == (4,) for i in cv["info"][k])
    # one fold again through glx.path: the same bits, and the loss of its own x with its own intercept
    tr, ho = sw.fold_vectors(np.arange(120) % 5, 2)
    out = glx.path(A, b, mus=cv["mus"], tol=1e-6, sample_weight=tr, holdout_weight=ho, fit_intercept=True)
    for i, (mu, x, info) in enumerate(out):
        assert info["holdout_loss"] == cv["fold_loss"][2, i]
        want = float(ic.holdout_loss(x, info["intercept"], A, b, ho))
        assert abs(info["holdout_loss"] - want) <= _holdout_bar(x, info["intercept"], A, b, ho, EPS64)


# ------------------------------------------------------------------------------------------ driver
def test_driver_intercept_lines():
    """python -m glx.driver --certified --intercept and --cv K --intercept: the tables are followed by
    one line each with the largest magnitude of the fitted intercepts."""
    from glx import driver
    fake = {"Fake": lambda x0, A, b, mu, opts: (np.zeros_like(x0), 3, {"tt": 0.0, "fval": 1.0})}
    out = io.StringIO()
    res = driver.run(dict(fake), stream=out, size=(40, 130, 3), seed=sw.SEED, certified="solve", cv=3, intercept=True)
    lines = out.getvalue().splitlines()
    cert = [ln for ln in lines if ln.startswith("# Intercept (certified): max |c| = ")]
    cvl = [ln for ln in lines if ln.startswith("# Intercept (cross-validation): max |c| over folds and mu = ")]
    assert len(cert) == 1 and len(cvl) == 1
    assert float(cert[0].split("=")[-1]) > 0.0
    want = max(float(np.max(np.abs(i["intercept"]))) for f in res["cv"]["info"] for i in f)
    assert abs(float(cvl[0].split("=")[-1]) - want) <= 1e-6 * want
    assert lines.index(cert[0]) < lines.index("# Cross-validation (3 folds)") < lines.index(cvl[0])
    assert any(ln.startswith("| Certified") for ln in lines)
    plain = io.StringIO()
    driver.run(dict(fake), stream=plain, size=(40, 130, 3), seed=sw.SEED, certified="solve")
    assert "Intercept" not in plain.getvalue()
