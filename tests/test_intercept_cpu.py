"""An unpenalised intercept without a device (DESIGN.md "Intercept"): the argument checks that must
raise before any device call, the two guards against their mirrors (tests/ic_ref.py), the safety of
the guarded test with centred norms at the reference solutions of the instances the GPU tests solve
(also with the record's gap forced to 0 and below), the reduction itself, and the reference curve of
the cross-validation instance.
"""
import ctypes

import numpy as np
import pytest

import group_ref as gr
import ic_ref as ic
import screen_ref as sr
import sw_ref as sw

LD = np.longdouble


# ------------------------------------------------------------------------------------------ arguments
def test_intercept_entries_refuse_before_any_device_work():
    """This machine may have no GPU: every call below must raise ValueError from the host checks."""
    import glx
    A, b = np.ones((4, 6)), np.ones((4, 2))
    x = np.zeros((6, 2))
    bads = ([1.0, 1.0, 1.0], [1.0, -1.0, 1.0, 1.0], [1.0, np.nan, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0], [0.0] * 4)
    for bad in bads:
        with pytest.raises(ValueError):
            glx.certificate(x, A, b, 0.1, sample_weight=bad, fit_intercept=True)
        with pytest.raises(ValueError):
            glx.mu_max(A, b, sample_weight=bad, fit_intercept=True)
        with pytest.raises(ValueError):
            glx.solve_certified(A, b, 0.1, sample_weight=bad, fit_intercept=True)
        with pytest.raises(ValueError):
            glx.solve_certified(A, b, 0.1, sample_weight=np.ones(4), holdout_weight=bad, fit_intercept=True)
        with pytest.raises(ValueError):
            glx.path(A, b, sample_weight=bad, fit_intercept=True)
        with pytest.raises(ValueError):
            glx.cv_path(A, b, folds=2, sample_weight=bad, fit_intercept=True)
    with pytest.raises(ValueError):
        glx.solve_certified(A, b, 0.1, groups=[0, 3, 5], fit_intercept=True)      # the groups' own check
    with pytest.raises(ValueError):
        glx.certificate(x, A, b, -1.0, fit_intercept=True)
    with pytest.raises(ValueError):
        glx.cv_path(A, b, folds=1, fit_intercept=True)
    with pytest.raises(TypeError):
        glx.path(A, b, fit_intercepts=True)


def test_c_entries_refuse_weight_sum_and_null_intercept_before_any_launch():
    """weight_sum not finite or <= 0 and intercept_out NULL are refused by the C entries themselves, ahead
    of every other use of their pointers: null device pointers never reach a launch here."""
    from glx import _lib
    h = _lib.lib()
    out8, hs, icpt = (ctypes.c_double * 8)(), ctypes.c_double(0.0), (ctypes.c_double * 2)()
    info, ginfo = _lib.GlxCertifiedInfo(), _lib.GlxGroupCertifiedInfo()
    p = _lib.GlxProblem(dtype=_lib.GLX_F64, method=0, m=4, n=6, l=2, A=None, b=None, x=None, mu0=0.1, comm=None)
    ptr = np.array([0, 2, 6], dtype=np.int32)
    gw = np.array([1.0, 2.0])
    cs = (ctypes.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    for sigma, ic_out in ((0.0, icpt), (-1.0, icpt), (float("nan"), icpt), (float("inf"), icpt), (4.0, None)):
        calls = [
            lambda: h.glx_certificate_ic(_lib.GLX_F64, 4, 6, 2, None, None, None, 0.1, 0, None, None, sigma, None,
                                         None, out8, ctypes.byref(hs), ic_out, None, 0, None),
            lambda: h.glx_group_certificate_ic(_lib.GLX_F64, 4, 6, 2, None, None, None, 0.1, 2, ptr.ctypes.data,
                                               gw.ctypes.data, None, None, sigma, None, None, out8,
                                               ctypes.byref(hs), ic_out, None, 0, None),
            lambda: h.glx_certified_solve_ic(ctypes.byref(p), None, None, sigma, 1.0, 1e-6, 10, 1, 10, None, None,
                                             None, None, 0, ctypes.byref(info), ctypes.byref(hs), ic_out, None),
            lambda: h.glx_group_certified_solve_ic(ctypes.byref(p), 2, ptr.ctypes.data, gw.ctypes.data, None, None,
                                                   sigma, 1.0, 1e-6, 10, 1, 10, None, None, None, None, None, 0,
                                                   ctypes.byref(ginfo), ctypes.byref(hs), ic_out, None),
        ]
        for call in calls:
            assert call() != 0
            msg = h.glx_last_error().decode()
            assert "intercept" in msg, msg
    out4 = (ctypes.c_double * 4)()
    for sigma in (0.0, -2.0, float("nan"), float("inf")):
        assert h.glx_screen_guard_ic(out8, 0.1, _lib.GLX_F64, 4, 6, 2, cs, 1.0, sigma, 0.0, out4) != 0
        assert h.glx_group_screen_guard_ic(out8, 0.1, _lib.GLX_F64, 4, 6, 2, 2, 1.0, 1.0, cs, 1.0, sigma, 0.0,
                                           out4) != 0
    # a hold-out vector without sample weights is the _sw entries' refusal and stays one
    assert h.glx_certificate_ic(_lib.GLX_F64, 4, 6, 2, None, None, None, 0.1, 0, None, ctypes.c_void_p(16), 4.0, None,
                                None, out8, ctypes.byref(hs), icpt, None, 0, None) != 0
    # the describe lines name the centring finalize
    buf = ctypes.create_string_buffer(2048)
    for fn, args in ((h.glx_certificate_ic_describe, (_lib.GLX_F64, 96, 512, 16, 0)),
                     (h.glx_group_certificate_ic_describe, (_lib.GLX_F64, 96, 512, 16, 5)),
                     (h.glx_certified_ic_describe, (_lib.GLX_F64, 96, 512, 16, 1)),
                     (h.glx_group_certified_ic_describe, (_lib.GLX_F64, 96, 512, 16, 5, 1))):
        assert fn(*args, buf, len(buf)) == 0
        assert "k_cert_csum" in buf.value.decode() and "k_cert_fin_c" in buf.value.decode()


def test_workspaces_keep_the_siblings_layout_in_front():
    """The _ic workspaces are the _sw ones with the new pieces behind: never smaller."""
    from glx import _lib
    h = _lib.lib()
    for (m, n, l) in ((96, 512, 16), (40, 130, 3)):
        a, c = ctypes.c_size_t(0), ctypes.c_size_t(0)
        _lib.check(h.glx_certificate_sw_workspace_bytes(_lib.GLX_F64, m, n, l, ctypes.byref(a)))
        _lib.check(h.glx_certificate_ic_workspace_bytes(_lib.GLX_F64, m, n, l, ctypes.byref(c)))
        assert c.value >= a.value + 8 * m * l + 8 * l
        _lib.check(h.glx_certified_sw_workspace_bytes(_lib.GLX_F64, m, n, l, 1, ctypes.byref(a)))
        _lib.check(h.glx_certified_ic_workspace_bytes(_lib.GLX_F64, m, n, l, 1, ctypes.byref(c)))
        assert c.value >= a.value + 8 * m * l + 8 * l + 8 * n


# ------------------------------------------------------------------------------------------ guards
def test_intercept_guards_equal_their_mirrors():
    from glx import _lib, kernels as k
    g = np.random.default_rng(23)
    for dtype, eps in ((_lib.GLX_F64, sr.EPS64), (_lib.GLX_F32, sr.EPS32)):
        for _ in range(50):
            m, n, l = int(g.integers(1, 5000)), int(g.integers(1, 20000)), int(g.integers(1, 129))
            rr = float(g.uniform(0.0, 10.0)) * float(g.choice([0.0, 1e-12, 1.0]))
            bn = float(g.uniform(0.0, 10.0))
            rb = float(g.uniform(-1.0, 1.0)) * np.sqrt(rr) * bn
            sx = float(g.uniform(0.0, 50.0))
            gmax = float(g.uniform(0.0, 2.0))
            mu = float(g.choice([0.0, 1e-3, 1.0, 5.0]))
            cmax = float(g.uniform(0.1, 100.0))
            csq = cmax * cmax * float(g.uniform(1.0, n))
            amax = float(g.uniform(0.0, 3.0))
            cst = [cmax, csq, amax, amax * amax * float(g.uniform(1.0, n))]
            sigma = float(g.uniform(0.5, 2.0)) * m
            msq = float(g.uniform(0.0, 4.0))
            rec = [rr, rb, sx, gmax, 0.0, 0.0, 0.0, 0.0]
            want = ic.guard(rec, mu, eps, m, n, l, cst, bn, sigma, msq)
            got = k.screen_guard_ic(rec, mu, dtype, m, n, l, cst, bn, sigma, msq)
            for a, v in zip(want, got):
                assert abs(v - a) <= 16 * sr.EPS64 * abs(a), (dtype, m, n, l, rec, mu, want, got)
            # never a larger scale or a smaller bound than the weighted guard on the same record
            ws = k.screen_guard_sw(rec, mu, dtype, m, n, l, cmax, csq, bn)
            assert got[0] <= ws[0] and got[1] >= ws[1] and got[3] >= 0.0
            max_run = int(g.integers(1, min(n, 70) + 1))
            w_min = float(g.uniform(0.1, 3.0))
            want = ic.group_guard(rec, mu, eps, m, n, l, max_run, w_min, cmax, cst, bn, sigma, msq)
            got = k.group_screen_guard_ic(rec, mu, dtype, m, n, l, max_run, w_min, cmax, cst, bn, sigma, msq)
            for a, v in zip(want, got):
                assert abs(v - a) <= 16 * sr.EPS64 * abs(a), (dtype, m, n, l, max_run, rec, mu, want, got)
    with pytest.raises(_lib.GlxError):
        k.screen_guard_ic([1.0] * 8, -1.0, _lib.GLX_F64, 10, 10, 2, [1.0, 10.0, 1.0, 10.0], 1.0, 10.0, 0.0)
    with pytest.raises(_lib.GlxError):
        k.group_screen_guard_ic([1.0] * 8, 0.1, _lib.GLX_F64, 10, 10, 2, 11, 1.0, 1.0, [1.0, 10.0, 1.0, 10.0], 1.0,
                                10.0, 0.0)
    out = k.screen_guard_ic([float("nan"), 0.0, 1.0, 1.0, 0, 0, 0, 0], 0.1, _lib.GLX_F64, 10, 10, 2,
                            [1.0, 10.0, 1.0, 10.0], 1.0, 10.0, 0.0)
    assert all(np.isnan(v) for v in out[1:])


ROW_CASES = [(m, n, l, ratio, kind) for (m, n, l) in ((96, 512, 16), (40, 130, 3)) for kind in ("ones", "general")
             for ratio in (0.5, 0.1)]


def _row_case(case):
    from glx import _lib
    m, n, l, ratio, kind = case
    ref = ic.reference_solution(m, n, l, ratio, kind)
    A, b, w, mu, x = ref["A"], ref["b"], ref["w"], ref["mu"], ref["x"]
    c = ic.certificate(x, A, b, mu, w, wide=np.float64)
    cn = np.asarray(ic.col_norms(A, w), dtype=np.float64)
    cst, bn, sigma = ic.figures(A, b, w)
    nz = np.sqrt(np.sum(x * x, axis=1)) != 0
    assert 0 < nz.sum() < n
    return {"m": m, "n": n, "l": l, "mu": mu, "c": c, "cn": cn, "cst": cst, "bn": bn, "sigma": sigma, "nz": nz,
            "msq": float(np.sum(c["intercept"] ** 2)), "dtype": _lib.GLX_F64}


def _row_screened(cs, rec):
    from glx import kernels as k
    s, gap_p, rho, slack = k.screen_guard_ic(rec, cs["mu"], cs["dtype"], cs["m"], cs["n"], cs["l"], cs["cst"],
                                             cs["bn"], cs["sigma"], cs["msq"])
    keep = sr.keep_mask(cs["c"]["row_norms"], cs["cn"], s, rho, cs["mu"] - slack)
    return s, gap_p, rho, slack, ~keep


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: "%dx%dx%d@%g-%s" % c)
@pytest.mark.parametrize("forced", [None, 0.0, -1e-9], ids=["as-is", "gap0", "gap-1e-9P"])
def test_intercept_guard_is_safe_at_xstar(case, forced):
    """The guarded test with CENTRED norms discards no row with x*_i != 0."""
    cs = _row_case(case)
    rec = sr.record(cs["c"])
    s0, gap_p, rho, slack, scr = _row_screened(cs, rec)
    if forced is None:
        assert rho > 0.0 and gap_p >= max(float(cs["c"]["gap"]), 0.0) and 0.0 < s0 <= 1.0
        assert 0.0 <= slack <= 1e-9 * cs["mu"]
        assert scr.sum() > 0                     # (x* is accurate enough to screen something)
    else:
        rr, rb, mu = rec[0], rec[1], cs["mu"]
        primal = 0.5 * rr + mu * rec[2]
        rec[2] = (forced * primal - (0.5 * (1.0 + s0 * s0) * rr + s0 * rb)) / mu
        s, gap_p, rho, slack, scr = _row_screened(cs, rec)
        assert s == s0 and rho > 0.0 and gap_p > 0.0
    assert not np.any(scr & cs["nz"])


@pytest.mark.parametrize("forced", [None, 0.0, -1e-9], ids=["as-is", "gap0", "gap-1e-9P"])
def test_intercept_group_guard_is_safe_at_xstar(forced):
    from glx import _lib, kernels as k
    m, n, l, ratio = 96, 512, 16, 0.5
    ref = ic.group_reference_solution(m, n, l, ratio)
    A, b, w, ptr, gw, mu, x = (ref[key] for key in ("A", "b", "w", "ptr", "gw", "mu", "x"))
    c = ic.certificate(x, A, b, mu, w, ptr, gw, wide=np.float64)
    Ac, _ = ic.centre(A, b, w)
    gcn = np.asarray(gr.group_cnorms(Ac, ptr, gw), dtype=np.float64)
    cst, bn, sigma = ic.figures(A, b, w)
    nz = gr.group_norms(x, ptr) != 0
    assert 0 < nz.sum() < nz.size
    rec = gr.record(c)
    args = (mu, _lib.GLX_F64, m, n, l, int(np.diff(ptr).max()), float(gw.min()), float(gcn.max()), cst, bn, sigma,
            float(np.sum(c["intercept"] ** 2)))
    s0, gap_p, rho, slack = k.group_screen_guard_ic(rec, *args)
    if forced is not None:
        primal = 0.5 * rec[0] + mu * rec[2]
        rec[2] = (forced * primal - (0.5 * (1.0 + s0 * s0) * rec[0] + s0 * rec[1])) / mu
        s, gap_p, rho, slack = k.group_screen_guard_ic(rec, *args)
        assert s == s0 and rho > 0.0 and gap_p > 0.0
    scr = ~gr.keep_mask(c["group_norms"], gcn, s0, rho, mu - slack)
    assert not np.any(scr & nz)
    if forced is None:
        assert scr.sum() > 0


# ------------------------------------------------------------------------------------------ the reduction
@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: "%dx%dx%d@%g-%s" % c)
def test_the_reduction(case):
    """In longdouble, P(x, c(x)) formed on the original A and b equals the centred pair's primal, c(x)
    minimises over c, the centred residual is orthogonal to 1~, and the support differs from the
    intercept-free problem's (a solve that ignored the flag cannot pass the GPU tests)."""
    m, n, l, ratio, kind = case
    ref = ic.reference_solution(m, n, l, ratio, kind)
    A, b, w, mu, x, c = (ref[key] for key in ("A", "b", "w", "mu", "x", "c"))
    cert = ic.certificate(x, A, b, mu, w)
    p0 = ic.primal(x, c, A, b, mu, w)
    assert abs(p0 - cert["primal"]) <= 1e-16 * abs(p0) * m
    g = np.random.default_rng(5)
    for _ in range(4):
        assert ic.primal(x, c + 1e-3 * g.standard_normal(l), A, b, mu, w) > p0
    assert float(np.max(np.abs(np.sqrt(w.astype(LD)) @ cert["r"]))) <= 1e-15 * float(np.sqrt(cert["rr"])) * m
    # the uncentred norms by Pythagoras, as the guard recovers them
    cn, am = ic.col_norms(A, w), ic.col_means(A, w)
    un = sw.col_norms(A, w)
    assert np.all(np.abs(un * un - (cn * cn + np.sum(w.astype(LD)) * am * am)) <= 1e-15 * un * un * m)
    plain, _ = sr.fista_screen(*sw.reduce(A, b, w), mu, tol=1e-12)
    assert set(np.nonzero(np.sum(plain * plain, axis=1))[0]) != set(np.nonzero(np.sum(x * x, axis=1))[0])


def test_cv_reference_indices_with_an_intercept():
    """The reference curve of the cross-validation instance with offsets and an intercept per fold
    (tests/test_gpu_intercept.py asserts these indices of the GPU's curve): best = 5 and one_se = 5 at
    1e-6. Margins of this curve: the runner-up mean is 5.2 % above the minimum, mean[4] is 0.77 % above
    the 1-SE threshold, and solving to 1e-8 instead moves a mean by at most 3.5e-5 relative."""
    A, b = ic.cv_instance()
    mus, fl = ic.cv_reference(A, b, tol=1e-6)
    mean, se, best, one = sw.cv_aggregate(fl)
    assert (best, one) == (5, 5)
    order = np.sort(mean)
    assert order[1] / order[0] - 1.0 > 0.04
    thr = mean[best] + se[best]
    assert mean[4] > thr * 1.005
