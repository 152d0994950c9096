"""Gap-safe screening without a device: the rounding guard (glx_screen_guard, host only) against
tests/screen_ref.py's formulae, the guard's safety at the stored x* of the default instance, the
path's grid and argument checks, and the C ABI's refusals.

Safety at x*. The record comes from certificate_ref in float64, the column figures from the
reference; the guarded test (s_safe, rho+ from the library; the comparison itself in longdouble)
must screen no row with x*_i != 0. The same must hold when the record's gap is forced to 0 and to a
small negative value (sum ||x_i|| is moved so that 1/2 (1 + s^2) rr + s rb + mu sx comes out 0, or
-1e-9 of the primal): DESIGN.md records a trial that flagged nonzero rows once the computed gap had
rounded to 0, and rho+ > 0 is what prevents it.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

import certificate_ref as cref
import screen_ref as sr


def _kernels():
    from glx import kernels
    return kernels


def test_guard_equals_reference_formulae():
    from glx import _lib
    k = _kernels()
    g = np.random.default_rng(7)
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
            rec = [rr, rb, sx, gmax, 0.0, 0.0, 0.0, 0.0]
            want = sr.guard(rec, mu, eps, m, n, l, cmax, csq, bn)
            got = k.screen_guard(rec, mu, dtype, m, n, l, cmax, csq, bn)
            for w, v in zip(want, got):
                assert abs(v - w) <= 8 * sr.EPS64 * abs(w), (dtype, m, n, l, rec, mu, want, got)
            assert 0.0 <= got[0] <= 1.0 and got[1] >= 0.0 and got[2] >= 0.0


def test_guard_propagates_nan_and_refuses_bad_arguments():
    from glx import _lib
    k = _kernels()
    out = k.screen_guard([float("nan"), 0.0, 1.0, 1.0, 0, 0, 0, 0], 0.1, _lib.GLX_F64, 10, 10, 2, 1.0, 10.0, 1.0)
    assert all(np.isnan(v) for v in out[1:])
    out = k.screen_guard([1.0, 0.0, 1.0, float("nan"), 0, 0, 0, 0], 0.1, _lib.GLX_F64, 10, 10, 2, 1.0, 10.0, 1.0)
    assert all(np.isnan(v) for v in out)
    with pytest.raises(_lib.GlxError):
        k.screen_guard([1.0] * 8, -1.0, _lib.GLX_F64, 10, 10, 2, 1.0, 10.0, 1.0)
    with pytest.raises(_lib.GlxError):
        k.screen_guard([1.0] * 8, 0.1, _lib.GLX_F64, 10, 10, 129, 1.0, 10.0, 1.0)
    with pytest.raises(_lib.GlxError):
        k.screen_guard([1.0] * 8, 0.1, 7, 10, 10, 2, 1.0, 10.0, 1.0)


@pytest.fixture(scope="module")
def at_xstar():
    from glx import _lib
    A, b, _, mu = cref.instance(97006855, 256, 512, 2)
    x = np.load(os.path.join(GOLDEN, "default_xstar.npz"))["x"]
    c = cref.certificate(x, A, b, mu)
    cn = np.asarray(sr.col_norms(A), dtype=np.float64)
    fig = (float(cn.max()), float(np.sum(cn * cn)), float(np.linalg.norm(b)))
    nz = np.sqrt(np.sum(x * x, axis=1)) != 0
    assert 0 < nz.sum() < 512
    return {"A": A, "b": b, "mu": mu, "x": x, "c": c, "cn": cn, "fig": fig, "nz": nz, "dtype": _lib.GLX_F64}


def _screened(case, rec):
    m, n = case["A"].shape
    s, gap_p, rho = _kernels().screen_guard(rec, case["mu"], case["dtype"], m, n, 2, *case["fig"])
    keep = sr.keep_mask(case["c"]["row_norms"], case["cn"], s, rho, case["mu"])
    return s, gap_p, rho, ~keep


def test_guard_is_safe_at_xstar(at_xstar):
    rec = sr.record(at_xstar["c"])
    s, gap_p, rho, scr = _screened(at_xstar, rec)
    assert rho > 0.0 and gap_p >= max(float(at_xstar["c"]["gap"]), 0.0) and 0.0 < s <= 1.0
    assert not np.any(scr & at_xstar["nz"])
    assert scr.sum() > 0                      # (x* is accurate enough to screen something)


@pytest.mark.parametrize("forced", [0.0, -1e-9])
def test_guard_is_safe_when_the_gap_rounds_to_zero_or_below(at_xstar, forced):
    c, mu = at_xstar["c"], at_xstar["mu"]
    rec = sr.record(c)
    s0 = _screened(at_xstar, rec)[0]
    rr, rb = rec[0], rec[1]
    primal = 0.5 * rr + mu * rec[2]
    rec[2] = (forced * primal - (0.5 * (1.0 + s0 * s0) * rr + s0 * rb)) / mu
    gap = 0.5 * (1.0 + s0 * s0) * rr + s0 * rb + mu * rec[2]
    assert abs(gap - forced * primal) <= 1e-12 * primal
    s, gap_p, rho, scr = _screened(at_xstar, rec)
    assert s == s0 and rho > 0.0 and gap_p > 0.0
    assert not np.any(scr & at_xstar["nz"])


def test_mu_grid_and_path_argument_checks():
    from glx.screen import mu_grid, path, solve_certified
    g = mu_grid(3.0, 4, 1e-3)
    assert g[0] == 3.0 and len(g) == 4 and abs(g[-1] - 3e-3) <= 1e-15
    assert all(b < a for a, b in zip(g, g[1:]))
    ratios = [b / a for a, b in zip(g, g[1:])]
    assert max(ratios) - min(ratios) <= 1e-14
    assert mu_grid(2.0, 1) == [2.0]
    for bad in (dict(n_mus=0), dict(mu_min_ratio=0.0), dict(mu_min_ratio=1.0), dict(mu_min_ratio=-1.0)):
        with pytest.raises(ValueError):
            mu_grid(1.0, **{"n_mus": 3, "mu_min_ratio": 0.1, **bad})
    with pytest.raises(ValueError):
        mu_grid(0.0)
    A, b = np.zeros((4, 6)), np.zeros((4, 2))
    # refused before any device work (this machine may have none)
    with pytest.raises(ValueError):
        path(A, np.zeros((5, 2)))
    with pytest.raises(ValueError):
        path(A, np.zeros(4))
    with pytest.raises(ValueError):
        path(A, b, mus=[1.0, 1.0])
    with pytest.raises(ValueError):
        path(A, b, mus=[1.0, 2.0])
    with pytest.raises(ValueError):
        path(A, b, mus=[1.0, -0.5])
    with pytest.raises(ValueError):
        path(A, b, mus=[])
    with pytest.raises(ValueError):
        path(A, b, n_mus=0)
    with pytest.raises(ValueError):
        path(A, b, mu_min_ratio=2.0)
    with pytest.raises(ValueError):
        path(A, b, tol=0.0)
    with pytest.raises(ValueError):
        path(A, b, check_every=0)
    with pytest.raises(TypeError):
        path(A, b, nonsense=1)
    with pytest.raises(ValueError):
        solve_certified(A, b, -1.0)
    with pytest.raises(ValueError):
        solve_certified(A, b, 1.0, x0=np.zeros((6, 3)))
    with pytest.raises(ValueError):
        solve_certified(A, b, 1.0, maxit=-1)


def test_c_abi_refusals_and_workspace():
    from glx import _lib
    h = _lib.lib()
    nb = ctypes.c_size_t(0)
    assert h.glx_certified_workspace_bytes(_lib.GLX_F64, 96, 512, 16, 1, ctypes.byref(nb)) == 0
    with_screen = nb.value
    assert h.glx_certified_workspace_bytes(_lib.GLX_F64, 96, 512, 16, 0, ctypes.byref(nb)) == 0
    # the two compaction buffers: at most 0.9 m n and 0.81 m n elements
    assert 0 < with_screen - nb.value <= int((0.9 + 0.81) * 96 * 512 * 8) + 4096
    assert h.glx_certified_workspace_bytes(_lib.GLX_F64, 96, 512, 129, 1, ctypes.byref(nb)) == 1
    assert h.glx_certified_workspace_bytes(_lib.GLX_F64, 96, 512, 16, 1, None) == 1
    assert h.glx_certified_workspace_bytes(5, 96, 512, 16, 1, ctypes.byref(nb)) == 1
    assert h.glx_screen_workspace_bytes(0, 5, ctypes.byref(nb)) == 1
    assert "screening=gap-safe" in _lib.certified_describe(_lib.GLX_F64, 96, 512, 16, True)
    assert "screening=off" in _lib.certified_describe(_lib.GLX_F32, 40, 130, 3, False)
    assert "row kernel" in _lib.certified_describe(_lib.GLX_F64, 40, 130, 3, True)

    P = 4096   # a fake, aligned pointer: every refusal below comes before the first device call
    info = _lib.GlxCertifiedInfo()

    def solve(dtype=_lib.GLX_F64, l=16, mu=0.1, comm=None, t=1e-3, tol=1e-6, maxit=10, every=10, A=P, ws=P,
              wsb=with_screen, cn=None, cs=None):
        p = _lib.GlxProblem(dtype=dtype, method=0, m=96, n=512, l=l, A=A, b=P, x=P, mu0=mu, comm=comm)
        return h.glx_certified_solve(ctypes.byref(p), t, tol, maxit, 1, every, cn, cs, None, ws, wsb,
                                     ctypes.byref(info), None)

    assert solve(comm=P) == 1 and b"single-GPU" in h.glx_last_error()
    assert solve(l=129) == 1
    assert solve(mu=-1.0) == 1
    assert solve(mu=float("nan")) == 1
    assert solve(t=0.0) == 1
    assert solve(tol=0.0) == 1
    assert solve(maxit=-1) == 1
    assert solve(every=0) == 1
    assert solve(A=None) == 1
    assert solve(A=P + 8) == 1
    assert solve(ws=None) == 1
    assert solve(ws=P + 16) == 1
    assert solve(wsb=with_screen - 1) == 1
    assert solve(cn=P) == 1                       # the norms without their figures
    assert h.glx_gather_cols(_lib.GLX_F64, 4, 8, P, P, 65, P, None) == 1
    assert h.glx_gather_cols(_lib.GLX_F64, 4, 8, None, P, 64, P, None) == 1
    assert h.glx_screen_step(0, P, P, 1.0, 1.0, 1.0, None, P, P, P, 1 << 20, None) == 1
    assert h.glx_col_norms(_lib.GLX_F64, 4, 8, None, P, P, P, 1 << 20, None) == 1
