"""The certified solve's loop and step on the GPU (glx.solve_certified; solve() in csrc/screen.cpp)
against tests/loop_ref.py, the NumPy model of that loop, and glx.solver._lambda_max against eigvalsh.

The other modules hold a whole solve to its fixed point. Here tol = 1e-30, so only maxit stops a
solve, and what is compared is the iterate after exactly K iterations, the counters of the loop and
every screening decision on the way.

a. Trajectories, screening off: K in {1, 3, 10, 25}, float64 and float32, from x0 = 0 and once from a
   random x0; the fused step (k_atr_fista), the row kernel (k_fista_trial), the group kernel (one
   group_ref.CASES instance per layout that describe names) and the weighted finalize (weights with
   zeros). In float32 the planner gives 96 x 512 the four-panel A^T r tile, which has no fused
   epilogue, so that shape runs the row kernel there; 96 x 320 is the float32 shape that fuses.
b. Trajectories through compactions, float64: the histories of loop_ref.LOOP_CASES, which
   tests/test_loop_ref_cpu.py pins with min_margin >= 1e-6 (so no decision is exempt); kept_history,
   compactions, width, kept, checks, rounds and kept_rows equal the model's, every row outside
   kept_rows is exactly +0, and the returned certificate is glx.certificate's of the returned x.
c. Branches: maxit = 0; maxit = 7; kept == 0 from a warm start (with and without compactions on the
   way); check_every in {1, 7, maxit + 5}.
d. The bar of an iterate is measured, not fixed: 16 d(K) + 4 eps_T max |x_LD| (loop_ref.x_bar), with
   d(K) the distance of the model run in the working dtype from the model run in longdouble. The
   factor 16 is a margin for the GPU's summation orders (MFMA tiles, K splits), a supposition. The
   mutations this module is for (a momentum index off by one, no restart or a stale y at a
   compaction) sit 10 or more orders above d(K) in float64 and 2 or more in float32.
   Worst err / bar per arm, measured on an MI355X (d(K) / max |x| was 2.9e-16 to 1.5e-15 in
   float64 and 9.5e-8 to 8.1e-7 in float32):
       a  fused        f64 0.156   f32 0.062      b  96x512x16@0.5      0.057
       a  row kernel   f64 0.148   f32 0.080      b  40x200x3@0.3       0.050   (ce=3: 0.043)
       a  groups       f64 0.072   f32 0.065      b  64x1024x16@0.5     0.049
       a  weights      f64 0.034   f32 0.042      b  groups 0.033, sample weights 0.052
       c  maxit=7: 0.057 (40x130x3), 0.137 (96x512x16); check_every 1: 0.054, 7 and maxit+5: 0.045
   With k + 3 for k + 2 in iterate() 28 of the cases of a to c fail; without k = 1 at a compaction,
   or without the copy of x to y there, 8 (all of b, and the two of c that compact more than once);
   with the final compose taking no map, 6 (kept_rows).
e. _lambda_max (the host Lanczos that gives every certified solve, path and fold its step) against
   eigvalsh(A^T W A)[-1] in float64 on spectra built from QR factors of seeded normals. A result
   returned without a warning is within 1e-12 relative; where max_steps runs out (a flat top of the
   spectrum) a RuntimeWarning names the steps and the Ritz residual, and the value is never above
   lambda_max (1 + 1e-12).
"""
import functools
import json
import warnings

import numpy as np
import pytest

import group_ref as gr
import loop_ref as lr
import screen_ref as sr

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS64 = sr.EPS64
TOL = 1e-30
CERT_KEYS = ("primal", "dual", "gap", "rel_gap", "scale", "gmax", "kkt_max", "kkt_fro")
MEASURED = {}


def _note(key, ratio):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nworst err / bar:", json.dumps({k: float("%.3g" % v) for k, v in sorted(MEASURED.items())}))


def _np_dt(f32):
    return np.float32 if f32 else np.float64


def _solve(p, f32, maxit, screen, check_every=10, x0=None):
    import glx
    dt = _np_dt(f32)
    kw = {}
    if p["ptr"] is not None:
        kw.update(groups=p["ptr"].copy(), weights=p["gw"].copy())
    if p["w"] is not None:
        kw["sample_weight"] = p["w"].copy()
    return glx.solve_certified(p["A"].astype(dt), p["b"].astype(dt), p["mu"], x0=None if x0 is None else x0.astype(dt),
                               tol=TOL, maxit=maxit, screen=screen, check_every=check_every, **kw)


def _certificate(p, x):
    import glx
    dt = x.dtype.type
    kw = {}
    if p["w"] is not None:
        kw["sample_weight"] = p["w"].copy()
    if p["ptr"] is not None:
        return glx.certificate(x, p["A"].astype(dt), p["b"].astype(dt), p["mu"], p["ptr"].copy(), p["gw"].copy(), **kw)
    return glx.certificate(x, p["A"].astype(dt), p["b"].astype(dt), p["mu"], **kw)


def _assert_certificate(p, x, info):
    cert = _certificate(p, x)
    keys = CERT_KEYS + (("nonzero_groups",) if p["ptr"] is not None else ("nonzero_rows",))
    for key in keys:
        assert info[key] == cert[key], key


def _check_step(p, info):
    lam = 1.0 / lr.step(p["A"], p["w"])
    assert abs(info["step"] * lam - 1.0) <= 1e-12, info["step"] * lam - 1.0


def _check_x(arm, x, x_T, x_ld, f32):
    """x (GPU) against the longdouble model's iterate under loop_ref.x_bar; prints and notes err / bar."""
    eps = sr.EPS32 if f32 else EPS64
    assert x.dtype == _np_dt(f32) and x.shape == x_ld.shape
    bar = lr.x_bar(x_T, x_ld, eps)
    err = float(np.max(np.abs(x.astype(LD) - x_ld)))
    print("%s: err %.3e, bar %.3e (d / max |x| %.2e), err / bar %.3f"
          % (arm, err, bar, float(np.max(np.abs(x_T.astype(LD) - x_ld)) / np.max(np.abs(x_ld))), err / bar))
    _note(arm.split(" K=")[0], err / bar)
    return err / bar


# ------------------------------------------------------------------------------------------ a
KS = (1, 3, 10, 25)
TRAJ = [(96, 512, 16, 0.5), (96, 512, 16, 0.1), (40, 130, 3, 0.1), (96, 320, 16, 0.5)]


def _plan_kernel(m, n, l, f32):
    if (m, n, l) == (40, 130, 3):
        return "k_fista_trial"
    if (m, n, l) == (96, 512, 16) and f32:    # the float32 four-panel A^T r tile has no fused epilogue
        return "k_fista_trial"
    return "k_atr_fista"


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", TRAJ, ids=lambda c: "%dx%dx%d@%g" % c)
def test_trajectory(case, f32):
    m, n, l, ratio = case
    key = ("rows", m, n, l, ratio, f32)
    p = lr.problem(*key)
    T = "f32" if f32 else "f64"
    arm = "a %s %s" % ("fused" if _plan_kernel(m, n, l, f32) == "k_atr_fista" else "row kernel", T)
    _, i_ld = lr.model(key, "ld", KS[-1], 10, False, None, KS)
    _, i_T = lr.model(key, T, KS[-1], 10, False, None, KS)
    worst = {}
    print()
    for K in KS:
        x, info = _solve(p, f32, K, False)
        assert info["iterations"] == K and not info["converged"] and info["compactions"] == 0
        assert info["checks"] == 2 + (K - 1) // 10 and info["rounds"] == 1 and info["width"] == n
        assert _plan_kernel(m, n, l, f32) in info["plan"], info["plan"]
        assert info["step_fused"] == ("k_atr_fista" in info["plan"])
        _check_step(p, info)
        worst[K] = _check_x("%s K=%d %s" % (arm, K, case), x, i_T["snapshots"][K], i_ld["snapshots"][K], f32)
    # once from a random nonzero x0
    x0 = lr.start(n, l, 0.1, f32)
    x_ld, _ = lr.model(key, "ld", 10, 10, False, 0.1)
    x_T, _ = lr.model(key, T, 10, 10, False, 0.1)
    x, info = _solve(p, f32, 10, False, x0=x0)
    assert info["iterations"] == 10 and not info["converged"]
    worst["x0"] = _check_x("%s K=10 x0 %s" % (arm, case), x, x_T, x_ld, f32)
    assert all(v <= 1 for v in worst.values()), worst


GROUP_ARMS = [gr.CASES[0], gr.CASES[2], gr.CASES[4]]


def test_group_arms_cover_the_layouts():
    """One instance per layout that describe names for group_ref.CASES (host only)."""
    from glx import _lib

    def layout(c):
        m, n, l, pool, _ = c
        ptr = gr.instance(gr.SEED, m, n, l, pool)[2]
        return _lib.group_certified_describe(_lib.GLX_F64, m, n, l, int(np.diff(ptr).max()), False).split("step=")[1]
    arms = [layout(c) for c in GROUP_ARMS]
    assert len(set(arms)) == len(arms) and set(arms) == {layout(c) for c in gr.CASES}
    assert sum("in registers" in a for a in arms) == 2


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", GROUP_ARMS, ids=lambda c: "%dx%dx%d-%s@%g" % (c[0], c[1], c[2], c[3][1], c[4]))
def test_trajectory_groups(case, f32):
    m, n, l, pool, ratio = case
    key = ("grp", m, n, l, ratio, f32, pool)
    p = lr.problem(*key)
    T = "f32" if f32 else "f64"
    x_ld, _ = lr.model(key, "ld", 10, 10, False)
    x_T, _ = lr.model(key, T, 10, 10, False)
    x, info = _solve(p, f32, 10, False)
    assert info["iterations"] == 10 and not info["converged"] and info["compactions"] == 0
    assert "k_group_fista" in info["plan"]
    _check_step(p, info)
    print()
    assert _check_x("a groups %s K=10 %s" % (T, case[:3] + (pool[1],)), x, x_T, x_ld, f32) <= 1


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_trajectory_sample_weights(f32):
    key = ("sw", 96, 512, 16, 0.5, f32)
    p = lr.problem(*key)
    assert np.count_nonzero(p["w"] == 0) == 96 // 4
    T = "f32" if f32 else "f64"
    x_ld, _ = lr.model(key, "ld", 10, 10, False)
    x_T, _ = lr.model(key, T, 10, 10, False)
    x, info = _solve(p, f32, 10, False)
    assert info["iterations"] == 10 and not info["converged"] and info["compactions"] == 0
    assert "k_cert_fin_w" in info["plan"]
    _check_step(p, info)
    print()
    assert _check_x("a sample weights %s K=10" % T, x, x_T, x_ld, f32) <= 1


# ------------------------------------------------------------------------------------------ b, c
COUNTERS = ("iterations", "kept_history", "compactions", "width", "kept", "checks", "rounds")


def _assert_loop(arm, case, certificate=True):
    name, key, maxit, check_every, x0_scale, want = case
    p = lr.problem(*key)
    n, l = p["A"].shape[1], p["b"].shape[1]
    x_ld, i_ld = lr.model(key, "ld", maxit, check_every, True, x0_scale)
    x_T, _ = lr.model(key, "f64", maxit, check_every, True, x0_scale)
    assert i_ld["kept_history"] == want and i_ld["min_margin"] >= 1e-6      # (pinned in test_loop_ref_cpu.py)
    x0 = None if x0_scale is None else lr.start(n, l, x0_scale)
    x, info = _solve(p, False, maxit, True, check_every, x0)
    print("\n%s: history %s, width %d, kept %d, checks %d, iterations %d; model %s, min_margin %.2e"
          % (name, info["kept_history"], info["width"], info["kept"], info["checks"], info["iterations"],
             i_ld["kept_history"], i_ld["min_margin"]))
    for k in COUNTERS:
        assert info[k] == i_ld[k], (k, info[k], i_ld[k])
    assert info["converged"] == i_ld["converged"]
    assert np.array_equal(info["kept_rows"], i_ld["kept_rows"])
    if p["ptr"] is not None:
        assert np.array_equal(info["kept_groups"], i_ld["kept_groups"])
    off = np.ones(n, dtype=bool)
    off[info["kept_rows"]] = False
    assert np.all(x[off] == 0) and not np.any(np.signbit(x[off]))            # exactly +0
    _check_step(p, info)
    if certificate:
        _assert_certificate(p, x, info)
    if np.any(x_ld != 0):
        assert _check_x("%s %s" % (arm, name), x, x_T, x_ld, False) <= 1
    return x, info


@pytest.mark.parametrize("case", lr.LOOP_CASES, ids=lambda c: c[0])
def test_loop_through_compactions(case):
    x, info = _assert_loop("b", case)
    assert not info["converged"] and info["compactions"] == len(case[5]) >= 1


def test_plans_of_the_compacted_widths():
    """What the first case's reduced problems run (host only): the fused step at every width."""
    from glx import _lib
    for w in (512, 384, 128, 64):
        assert "k_atr_fista" in _lib.certified_describe(_lib.GLX_F64, 96, w, 16, True)
    assert "k_fista_trial" in _lib.certified_describe(_lib.GLX_F64, 40, 200, 3, True)


@pytest.mark.parametrize("screen", [True, False], ids=["screen", "noscreen"])
def test_maxit_zero(screen):
    import glx
    key = ("rows", 40, 130, 3, 0.1)
    p = lr.problem(*key)
    x0 = lr.start(130, 3, 1.0)
    _, i_ld = lr.model(key, "ld", 0, 10, screen, 1.0)
    assert i_ld["compactions"] == 0 and i_ld["checks"] == 1
    x, info = _solve(p, False, 0, screen, x0=x0)
    assert x.tobytes() == x0.tobytes()
    for k in COUNTERS:
        assert info[k] == i_ld[k], k
    assert not info["converged"] and np.array_equal(info["kept_rows"], np.arange(130))
    cert = glx.certificate(x0.copy(), p["A"].copy(), p["b"].copy(), p["mu"])
    for key_ in CERT_KEYS + ("nonzero_rows",):
        assert info[key_] == cert[key_], key_


@pytest.mark.parametrize("shape", [(40, 130, 3, 0.1), (96, 512, 16, 0.5)], ids=lambda c: "%dx%dx%d@%g" % c)
def test_maxit_exhausted(shape):
    case = ("maxit=7 %dx%dx%d" % shape[:3], ("rows",) + shape, 7, 10, None, [])
    x, info = _assert_loop("c", case)
    assert info["iterations"] == 7 and not info["converged"] and info["checks"] == 2


@pytest.mark.parametrize("case", lr.BRANCH_CASES, ids=lambda c: c[0])
def test_branches(case):
    name, key, maxit, check_every, x0_scale, want = case
    x, info = _assert_loop("c", case)
    if want[-1:] == [0]:        # kept == 0 from a warm start
        p = lr.problem(*key)
        assert np.all(x == 0) and not np.any(np.signbit(x))
        assert info["kept"] == 0 and info["kept_rows"].size == 0 and info["converged"] and info["width"] == 0
        half = float(np.sum(p["b"].astype(LD) ** 2) / 2)
        assert abs(info["primal"] - half) <= 33 * EPS64 * 2 * half      # (test_gpu_certificate's bar of ||r||^2)
        assert info["gap"] == 0.0
    else:
        assert info["iterations"] == maxit and not info["converged"]


# ------------------------------------------------------------------------------------------ e
def _factors(seed, m, n, r):
    g = np.random.default_rng(seed)
    U = np.linalg.qr(g.standard_normal((m, r)))[0]
    V = np.linalg.qr(g.standard_normal((n, r)))[0]
    return U, V


def _from_spectrum(seed, m, n, s):
    s = np.asarray(s, dtype=np.float64)
    U, V = _factors(seed, m, n, s.size)
    return (U * s) @ V.T


def _quarter_zero(seed, m):
    g = np.random.default_rng(seed)
    w = g.uniform(0.5, 3.0, m)
    w[g.choice(m, size=m // 4, replace=False)] = 0.0
    return w


def _lanczos_cases():
    """name -> (A, sample weights or None, dtype, max_steps, may_warn)."""
    g = np.random.default_rng(42)
    x = np.linspace(0.0, 1.0, 500)
    s20 = np.concatenate((1.0 - 1e-6 * np.linspace(0.0, 1.0, 20), np.linspace(0.9, 0.1, 44)))
    zc = g.standard_normal((50, 80))
    zc[:, ::7] = 0.0
    out = {
        "flat top x^4 n=500": (_from_spectrum(1, 500, 500, 1.0 - 0.999 * x ** 4), None, np.float64, 400, True),
        "linspace 600, 60 steps": (_from_spectrum(2, 600, 600, np.linspace(1e-3, 1.0, 600)), None, np.float64, 60, True),
        "random 40x130": (g.standard_normal((40, 130)), None, np.float64, 400, False),
        "random 64x1024": (g.standard_normal((64, 1024)), None, np.float64, 400, False),
        "random 64x1024 f32": (g.standard_normal((64, 1024)), None, np.float32, 400, False),
        "n=1": (g.standard_normal((30, 1)), None, np.float64, 400, False),
        "n=3": (g.standard_normal((30, 3)), None, np.float64, 400, False),
        "zero columns": (zc, None, np.float64, 400, False),
        "rank 1": (_from_spectrum(3, 60, 90, [2.5]), None, np.float64, 400, False),
        "pair 1e-10 apart": (_from_spectrum(4, 80, 120, np.concatenate(([1.0, 1.0 - 1e-10], np.linspace(0.8, 0.1, 30)))),
                             None, np.float64, 400, False),
        "20 within 1e-6": (_from_spectrum(5, 100, 150, s20), None, np.float64, 400, False),
        "weights with zeros": (g.standard_normal((96, 200)), _quarter_zero(6, 96), np.float64, 400, False),
        "weights with zeros m<n f32": (g.standard_normal((64, 320)), _quarter_zero(7, 64), np.float32, 400, False),
    }
    return out


LANCZOS = ["flat top x^4 n=500", "linspace 600, 60 steps", "random 40x130", "random 64x1024", "random 64x1024 f32",
           "n=1", "n=3", "zero columns", "rank 1", "pair 1e-10 apart", "20 within 1e-6", "weights with zeros",
           "weights with zeros m<n f32"]


@functools.lru_cache(maxsize=None)
def _lanczos_case(name):
    return _lanczos_cases()[name]


@pytest.mark.parametrize("name", LANCZOS)
def test_lambda_max(name):
    import torch
    from glx.solver import _lambda_max
    A, w, dt, max_steps, may_warn = _lanczos_case(name)
    A = A.astype(dt)
    wd = None if w is None else torch.as_tensor(w.astype(dt), device="cuda")
    A64 = A.astype(np.float64)
    At = A64 if w is None else np.sqrt(w.astype(dt).astype(np.float64))[:, None] * A64
    want = float(np.linalg.eigvalsh(At.T @ At)[-1])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = float(_lambda_max(torch.as_tensor(A, device="cuda"), max_steps=max_steps, sample_weight=wd))
    warned = [r for r in rec if issubclass(r.category, RuntimeWarning)]
    rel = (got - want) / want
    print("\n%s: lambda_max %.17g, got - want %.3e relative, %d warning(s)%s"
          % (name, want, rel, len(warned), "".join(": " + str(r.message) for r in warned)))
    assert got <= want * (1.0 + 1e-12)
    if may_warn:
        assert warned or abs(rel) <= 1e-12
        for r in warned:
            assert "%d steps" % max_steps in str(r.message) and "residual" in str(r.message)
    else:
        assert not warned
    if not warned:
        assert abs(rel) <= 1e-12


def test_lambda_max_warning_reaches_the_callers(monkeypatch):
    """_Prepared.set_weights (every certified solve, path and fold) and Session.__init__ (SGD / GD with
    continuous_subgradient_flag) let the warning through."""
    import glx
    import torch
    from glx import solver
    A = _lanczos_case("linspace 600, 60 steps")[0]
    b = np.random.default_rng(8).standard_normal((600, 2))
    monkeypatch.setattr(solver, "_lambda_max", functools.partial(solver._lambda_max, max_steps=60))
    with pytest.warns(RuntimeWarning, match="60 steps"):
        x, info = glx.solve_certified(A, b, 0.5 * glx.mu_max(A, b), maxit=0)
    assert info["step"] >= 1.0          # (lambda_max = 1: the step taken from a low Ritz value is above 1 / L)
    Ad, bd = torch.as_tensor(A, device="cuda"), torch.as_tensor(b, device="cuda")
    xd = torch.zeros((600, 2), dtype=torch.float64, device="cuda")
    with pytest.warns(RuntimeWarning, match="60 steps"):
        s = solver.Session("gl_GD_primal", xd, Ad, bd, 0.01, {"continuous_subgradient_flag": True})
    del s
