"""The sparse-group lasso without a GPU: tests/sgl_ref.py on its own, the refusals of the public interface
(raised before any device work) and the host-only guard glx_sgl_screen_guard against its mirror."""
import numpy as np
import pytest

import group_ref as gr
import sgl_ref as sr

LD = sr.LD
TAUS = [0.3, 0.9, 1.0]


def _instance(seed=3, m=30, n=47, l=3, pool=gr.POOL_RAGGED):
    return sr.instance(seed, m, n, l, pool)


@pytest.mark.parametrize("tau", [0.0] + TAUS)
def test_prox_minimises(tau):
    """F(x) = 1/2 ||x - w||^2 + t mu Omega_tau(x) is convex: no perturbation of the prox, small or large,
    along coordinates, rows, groups or at random, goes below it."""
    g = np.random.default_rng(5)
    _, _, ptr, w = _instance()
    n, l = int(ptr[-1]), 3
    wv = g.standard_normal((n, l)).astype(LD)
    tmu = LD(0.9)
    ta, tcw = LD(tau) * tmu, LD(1 - tau) * tmu * w.astype(LD)

    def F(x):
        return np.sum((x - wv) ** 2) / 2 + tmu * sr.omega(x, ptr, w, tau)

    p = sr.prox(wv, ta, tcw, ptr)
    f0 = F(p)
    assert np.any(sr.row_norms(p) == 0) and np.any(sr.row_norms(p) != 0)   # the case has both kinds of rows
    for scale in (1e-6, 1e-3, 1e-1):
        for _ in range(40):
            d = g.standard_normal((n, l)).astype(LD) * scale
            kind = g.integers(3)
            if kind == 1:   # one row only
                keep = np.zeros(n, dtype=bool)
                keep[g.integers(n)] = True
                d = d * keep[:, None]
            elif kind == 2:   # one group only
                k = g.integers(ptr.size - 1)
                keep = np.zeros(n, dtype=bool)
                keep[ptr[k]:ptr[k + 1]] = True
                d = d * keep[:, None]
            assert F(p + d) >= f0 - 1e-17 * abs(f0)


def test_tau0_is_the_group_reference():
    A, b, ptr, w = _instance()
    g = np.random.default_rng(1)
    wv = g.standard_normal((A.shape[1], b.shape[1]))
    tmuw = 0.8 * w
    # (equal up to the order of the norm's sum: q_g is the root of a sum of squared roots here)
    assert np.allclose(sr.prox(wv, 0.0, tmuw, ptr), gr.prox(wv, tmuw, ptr), rtol=1e-12, atol=1e-15)
    assert np.array_equal(sr.prox(wv, 0.0, tmuw, ptr) == 0, gr.prox(wv, tmuw, ptr) == 0)
    x = gr.prox(wv, tmuw, ptr)
    mu = 0.4 * gr.mu_max(A, b, ptr, w)
    c0, cg = sr.certificate(x, A, b, mu, ptr, w, 0.0), gr.certificate(x, A, b, mu, ptr, w)
    # (kkt_max is not compared: a nonzero group's distance is taken row by row here, so only the squares add up)
    for key in ("primal", "dual", "gap", "kkt_sq"):
        assert float(c0[key]) == pytest.approx(float(cg[key]), rel=1e-12, abs=1e-12), key
    assert c0["nonzero_groups"] == cg["nonzero_groups"]
    assert sr.mu_max(A, b, ptr, w, 0.0) == pytest.approx(gr.mu_max(A, b, ptr, w), rel=1e-14)


def test_tau1_is_the_row_problem():
    A, b, ptr, w = _instance()
    g = np.random.default_rng(2)
    wv = g.standard_normal((A.shape[1], b.shape[1]))
    nrm = sr.row_norms(wv)
    rowprox = wv * np.maximum(1 - 0.8 / nrm, 0)[:, None]
    assert np.allclose(sr.prox(wv, 0.8, 0.0 * w, ptr), rowprox, rtol=1e-13, atol=0)
    x = rowprox
    gmax = float(np.max(sr.row_norms(A.T @ b)))
    assert sr.mu_max(A, b, ptr, w, 1.0) == pytest.approx(gmax, rel=1e-14)
    mu = 0.4 * gmax
    c = sr.certificate(x, A, b, mu, ptr, w, 1.0)
    gi = sr.row_norms(c["g"])
    assert float(c["s_min"]) == pytest.approx(mu / float(np.max(gi)), rel=1e-14)
    xn = sr.row_norms(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        kk = np.where(xn != 0, sr.row_norms(c["g"] + mu * x / np.where(xn != 0, xn, 1)[:, None]), np.maximum(gi - mu, 0))
    assert float(c["kkt_max"]) == pytest.approx(float(np.max(kk)), rel=1e-12)
    assert c["nonzero_rows"] == int(np.sum(xn != 0))


@pytest.mark.parametrize("tau", [0.0, 0.3, 0.9])
def test_exact_s_is_the_supremum(tau):
    g = np.random.default_rng(7)
    for pool in (gr.POOL_SMALL, gr.POOL_LONG):
        ptr = gr.draw_groups(g, 300, pool)
        w = np.sqrt(np.diff(ptr).astype(np.float64))
        rho = np.abs(g.standard_normal(300)) * (g.random(300) < 0.8)
        rho[ptr[1]:ptr[2]] = 0.0
        a, cb = tau * 0.7, (1 - tau) * 0.7
        sg = sr.exact_sg(rho, ptr, w, a, cb)
        assert np.isinf(sg[1])
        for k in range(ptr.size - 1):
            if not np.isfinite(sg[k]):
                continue
            r, c = rho[ptr[k]:ptr[k + 1]].astype(LD), LD(cb) * LD(w[k])
            assert sr.phi(sg[k], r, LD(a)) <= c * (1 + LD(1e-15))
            assert sr.phi(sg[k] * (1 + LD(1e-9)), r, LD(a)) > c
        # the bracket's upper end (a + c_g) / max rho is never below the supremum
        pm = np.maximum.reduceat(rho, np.asarray(ptr[:-1], dtype=np.intp)).astype(LD)
        fin = np.isfinite(sg)
        assert np.all(sg[fin] <= (LD(a) + LD(cb) * w[fin]) / pm[fin] * (1 + LD(1e-15)))


@pytest.mark.parametrize("tau", TAUS)
def test_mu_max_is_where_zero_becomes_optimal(tau):
    A, b, ptr, w = _instance()
    top = sr.mu_max(A, b, ptr, w, tau)
    x0 = np.zeros((A.shape[1], b.shape[1]), dtype=LD)
    at = sr.certificate(x0, A.astype(LD), b.astype(LD), LD(top) * (1 + LD(1e-12)), ptr, w, tau)
    assert float(at["kkt_max"]) == 0.0 and float(at["scale"]) == 1.0 and abs(float(at["gap"])) <= 1e-25 * float(at["primal"])
    below = sr.certificate(x0, A.astype(LD), b.astype(LD), LD(0.999 * top), ptr, w, tau)
    assert float(below["kkt_max"]) > 0.0 and float(below["scale"]) < 1.0 and float(below["gap"]) > 0.0


def test_reference_solution_is_sparse_inside_groups():
    ref = sr.reference_solution(*sr.CASES[1])
    xg =gr.group_norms(ref["x"], ref["ptr"]) != 0
    inside = gr.expand_rows(xg, ref["ptr"]) & ~ref["support"]
    assert xg.any() and inside.any()   # a selected group with a zero row: what groups= alone cannot give
    x2, info = sr.fista_screen(ref["A"], ref["b"], ref["mu"], ref["ptr"], ref["w"], ref["tau"], tol=1e-10, screen=False)
    assert np.max(np.abs(x2 - ref["x"])) <= 1e-4 * np.max(np.abs(ref["x"]))
    hist = sr.fista_screen(ref["A"], ref["b"], ref["mu"], ref["ptr"], ref["w"], ref["tau"], tol=1e-10)[1]
    assert np.all(hist["kept_rows"][ref["support"]]) and hist["kept_row_history"] == sorted(hist["kept_row_history"])[::-1]


def test_refusals_need_no_device():
    import glx
    from glx.certificate import check_row_ratio
    A, b, ptr, w = _instance()
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="row_ratio"):
            glx.certificate(None, A, b, 1.0, groups=ptr, row_ratio=bad)
        with pytest.raises(ValueError, match="row_ratio"):
            glx.mu_max(A, b, groups=ptr, row_ratio=bad)
        with pytest.raises(ValueError, match="row_ratio"):
            glx.solve_certified(A, b, 1.0, groups=ptr, row_ratio=bad)
        with pytest.raises(ValueError, match="row_ratio"):
            glx.path(A, b, groups=ptr, row_ratio=bad)
        with pytest.raises(ValueError, match="row_ratio"):
            glx.cv_path(A, b, folds=3, groups=ptr, row_ratio=bad)
    for fn in (lambda: glx.certificate(None, A, b, 1.0, row_ratio=0.5), lambda: glx.mu_max(A, b, row_ratio=0.5),
               lambda: glx.solve_certified(A, b, 1.0, row_ratio=0.5), lambda: glx.path(A, b, row_ratio=0.5),
               lambda: glx.cv_path(A, b, folds=3, row_ratio=0.5)):
        with pytest.raises(ValueError, match="groups"):
            fn()
    for fn in (lambda: glx.certificate(None, A, b, 1.0, groups=ptr, row_ratio=0.5, fit_intercept=True),
               lambda: glx.mu_max(A, b, groups=ptr, row_ratio=0.5, fit_intercept=True),
               lambda: glx.solve_certified(A, b, 1.0, groups=ptr, row_ratio=0.5, fit_intercept=True),
               lambda: glx.path(A, b, groups=ptr, row_ratio=0.5, fit_intercept=True),
               lambda: glx.cv_path(A, b, folds=3, groups=ptr, row_ratio=0.5, fit_intercept=True)):
        with pytest.raises(ValueError, match="fit_intercept.*row_ratio|row_ratio.*fit_intercept"):
            fn()
    assert check_row_ratio(None, None) == 0.0 and check_row_ratio(0, (ptr, w)) == 0.0
    assert check_row_ratio(1, (ptr, w)) == 1.0 and check_row_ratio(0.0, (ptr, w), True) == 0.0


def test_driver_row_ratio_is_checked_first():
    from glx import driver
    with pytest.raises(ValueError, match="row_ratio"):
        driver.run(solvers={}, certified="solve", row_ratio=2.0)
    with pytest.raises(ValueError, match="fit_intercept"):
        driver.run(solvers={}, certified="solve", row_ratio=0.5, intercept=True)
    d = driver.demo_groups(10)
    assert list(d["groups"]) == [0, 4, 8, 10] and np.allclose(d["weights"] ** 2, [4, 4, 2])


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "sw"])
@pytest.mark.parametrize("eps,dtype", [(sr.EPS64, 1), (sr.EPS32, 0)], ids=["f64", "f32"])
def test_guard_equals_the_mirror(eps, dtype, weighted):
    from glx import _lib, kernels
    gdt = _lib.GLX_F64 if dtype == 1 else _lib.GLX_F32
    g = np.random.default_rng(11)
    for tau in TAUS:
        for _ in range(20):
            m, n, l, max_run = int(g.integers(1, 5000)), int(g.integers(8, 9000)), int(g.integers(1, 129)), int(g.integers(1, 9))
            rr, om = float(g.uniform(0, 50)), float(g.uniform(0, 30))
            rec = [rr, float(g.uniform(-1, 1)) * rr, om, 0.0, 0.0, 0.0, 0.0, 0.0]
            s_pad, mu = float(g.uniform(0.1, 2.0)), float(g.uniform(0.01, 5))
            args = (max_run, float(g.uniform(0.5, 2)), float(g.uniform(1, 80)), float(g.uniform(10, 1e5)), float(g.uniform(1, 60)))
            got = kernels.sgl_screen_guard(rec, s_pad, mu, tau, gdt, m, n, l, *args, weighted=weighted)
            want = sr.guard(rec, s_pad, mu, tau, eps, m, n, l, *args, weighted=weighted)
            assert np.allclose(got, want, rtol=1e-13, atol=0), (got, want)
            assert got[0] > 1.0 and got[1] >= 0.0 and got[2] == min(1.0, s_pad)
            assert got[3] >= max(0.0, 0.5 * (1 + got[2] ** 2) * rr + got[2] * rec[1] + mu * om)
    nan = kernels.sgl_screen_guard([float("nan")] + rec[1:], 0.5, 1.0, 0.3, gdt, 10, 20, 3, 2, 1.0, 2.0, 9.0, 1.0,
                                   weighted=weighted)
    assert np.isnan(nan[3]) and np.isnan(nan[4])
    with pytest.raises(_lib.GlxError):
        kernels.sgl_screen_guard(rec, 0.5, 1.0, 1.5, gdt, 10, 20, 3, 2, 1.0, 2.0, 9.0, 1.0)
