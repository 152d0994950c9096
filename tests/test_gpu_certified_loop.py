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
   The intercept arm (fit_intercept: k_cert_csum and k_cert_fin_c between the two dense passes, the step
   from _lambda_max(center_sum)) with sample weights, without and with groups, and the sparse-group arm
   (row_ratio: launch_atr then k_sgl_fista) at tau in {0.3, 0.9 with runs of 64 and 65 rows, 1} and with
   sample weights, at K = 10; one of each also at every K and from a random x0. With an intercept
   info["intercept"] is held to the model's in the same way: 16 times the distance of the working-dtype
   model's intercept from the longdouble one's plus 4 eps max |c|.
b. Trajectories through compactions, float64: the histories of loop_ref.LOOP_CASES, which
   tests/test_loop_ref_cpu.py pins with min_margin >= 1e-6 (so no decision is exempt); kept_history,
   compactions, width, kept, checks, rounds and kept_rows equal the model's, every row outside
   kept_rows is exactly +0, and the returned certificate is glx.certificate's of the returned x (with
   an intercept, "intercept" included). The sparse-group cases compare kept_row_history as well
   (never below kept_history, which counts groups) and nonzero_rows with the count on the returned x.
c. Branches: maxit = 0 (in the two later arms too); maxit = 7; kept == 0 from a warm start (with and
   without compactions on the way; with an intercept; in the sparse-group arm); check_every in
   {1, 7, maxit + 5}. With an intercept the certificate of x = 0 is not exactly 0: it sums w r_c^2 and
   w r_c b on r_c = fl(b-bar - b), so its gap is rounding dust of either sign (measured -1.5e-11,
   against a bar of 1.0e-7) and `converged` at tol = 1e-30 follows that sign; the test bounds the dust and
   compares every counter and decision as elsewhere.
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
   The intercept and sparse-group arms, under the same bar (the offset data's cancellation is in d(K)):
       a  ic weights   f64 0.050   f32 0.078      intercept  f64 0.053   f32 0.053
       a  ic           f64 0.048   f32 0.058      intercept  f64 0.035   f32 0.048
       a  ic groups    f64 0.049   f32 0.049      intercept  f64 0.047   f32 0.048
       a  sgl tau=0.3  f64 0.210   f32 0.079      a  sgl tau=0.9 long  f64 0.108   f32 0.065
       a  sgl tau=1    f64 0.070   f32 0.038      a  sgl weights       f64 0.057   f32 0.051
       b  ic weights 0.021, ic 0.033, ic ce=3 0.097, ic groups 0.046
       b  sgl tau=0.3 0.066 (l=16: 0.065), tau=0.9 long 0.047, tau=1 0.038, weights 0.066, ce=3 0.038
   With k + 3 for k + 2 in iterate() 28 of the cases of a to c fail; without k = 1 at a compaction,
   or without the copy of x to y there, 8 (all of b, and the two of c that compact more than once);
   with the final compose taking no map, 6 (kept_rows).
   Of the 29 cases of the two later arms (14 of a, 10 of b, 5 of c), tried one mutation of screen.cpp at
   a time: k + 3 for k + 2 in iterate() fails 26; no k = 1 at a compaction 11 (all of b, ic kept=0-ce=1);
   no copy of x to y there 12 (those, and sgl kept=0); cn not gathered in the sparse-group arm 3 (sgl
   tau=0.3, tau=1, ce=3); gside never flipped 3 (sgl tau=0.9 long, tau=1, ce=3).
e. _lambda_max (the host Lanczos that gives every certified solve, path and fold its step) against
   eigvalsh(A^T W A)[-1] in float64 on spectra built from QR factors of seeded normals. A result
   returned without a warning is within 1e-12 relative; where max_steps runs out (a flat top of the
   spectrum) a RuntimeWarning names the steps and the Ritz residual, and the value is never above
   lambda_max (1 + 1e-12). With center_sum (the intercept's step) the reference is eigvalsh of the
   centred weighted Gram matrix A^T W P A, P = I - 1 w^T / sigma, under the same rule: no weights and
   column offsets 5 times the columns' spread, weights with a quarter zeros, float32 A with m < n.
"""
import functools
import json
import warnings

import numpy as np
import pytest

import group_ref as gr
import ic_ref as icr
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
    kw.update(_arm_kw(p))
    return glx.solve_certified(p["A"].astype(dt), p["b"].astype(dt), p["mu"], x0=None if x0 is None else x0.astype(dt),
                               tol=TOL, maxit=maxit, screen=screen, check_every=check_every, **kw)


def _arm_kw(p):
    """The keywords of the two later arms: fit_intercept ("ic"), row_ratio ("tau"); none for the others."""
    kw = {}
    if p.get("ic"):
        kw["fit_intercept"] = True
    if p.get("tau") is not None:
        kw["row_ratio"] = p["tau"]
    return kw


def _certificate(p, x):
    import glx
    dt = x.dtype.type
    kw = _arm_kw(p)
    if p["w"] is not None:
        kw["sample_weight"] = p["w"].copy()
    if p["ptr"] is not None:
        return glx.certificate(x, p["A"].astype(dt), p["b"].astype(dt), p["mu"], p["ptr"].copy(), p["gw"].copy(), **kw)
    return glx.certificate(x, p["A"].astype(dt), p["b"].astype(dt), p["mu"], **kw)


def _assert_certificate(p, x, info):
    cert = _certificate(p, x)
    keys = CERT_KEYS + (("nonzero_groups",) if p["ptr"] is not None else ("nonzero_rows",))
    if p.get("tau") is not None:
        keys += ("nonzero_rows",)
    for key in keys:
        assert info[key] == cert[key], key
    if p.get("ic"):
        assert np.array_equal(info["intercept"], cert["intercept"])


def _check_step(p, info):
    """The step against the arm's own operator: A^T W A, or with an intercept the centred weighted Gram matrix."""
    if p.get("ic"):
        Ac = icr.centre(p["A"], p["b"], np.ones(p["A"].shape[0]) if p["w"] is None else p["w"])[0]
        lam = float(np.linalg.eigvalsh(Ac.T @ Ac)[-1])
    else:
        lam = 1.0 / lr.step(p["A"], p["w"])
    assert abs(info["step"] * lam - 1.0) <= 1e-12, info["step"] * lam - 1.0


def _check_intercept(arm, info, i_T, i_ld, f32):
    """info["intercept"] (GPU) against the longdouble model's, in loop_ref.x_bar's way: 16 times the distance of
    the working-dtype model's from it plus 4 eps max |c|."""
    eps = sr.EPS32 if f32 else EPS64
    c, c_T, c_ld = info["intercept"], i_T["intercept"], i_ld["intercept"]
    assert c.dtype == np.float64 and c.shape == c_ld.shape
    bar = 16.0 * float(np.max(np.abs(c_T - c_ld))) + 4.0 * eps * float(np.max(np.abs(c_ld)))
    err = float(np.max(np.abs(c.astype(LD) - c_ld)))
    print("%s intercept: err %.3e, bar %.3e, err / bar %.3f" % (arm, err, bar, err / bar))
    _note(arm.split(" K=")[0] + " intercept", err / bar)
    return err / bar


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


def _key32(key, f32):
    return key[:5] + (f32,) + key[6:]


def _plan_words(p):
    return ("k_cert_csum", "k_cert_fin_c") if p.get("ic") else ("k_sgl_fista",)


# (arm, problem key in float64, also at every K of KS and from a random x0)
ARM_TRAJ = [
    ("ic weights", ("ic", 96, 512, 16, 0.5, False, None, None, "general"), True),
    ("ic", ("ic", 96, 512, 16, 0.5, False), False),
    ("ic groups", ("icg", 96, 512, 16, 0.7, False, None, None, "general"), False),
    ("sgl tau=0.3", ("sgl", 96, 512, 16, 0.5, False, gr.POOL_SMALL, 0.3), True),
    ("sgl tau=0.9 long", ("sgl", 96, 512, 16, 0.5, False, gr.POOL_LONG, 0.9), False),
    ("sgl tau=1", ("sgl", 96, 512, 16, 0.5, False, gr.POOL_SMALL, 1.0), False),
    ("sgl weights", ("sgl", 96, 512, 16, 0.5, False, gr.POOL_SMALL, 0.3, "general"), False),
]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ARM_TRAJ, ids=lambda c: c[0])
def test_trajectory_intercept_and_sparse_group(case, f32):
    """The iterate after exactly K iterations of the intercept and the sparse-group arms, screening off."""
    name, key, every_k = case
    key = _key32(key, f32)
    p = lr.problem(*key)
    T = "f32" if f32 else "f64"
    arm = "a %s %s" % (name, T)
    ks = KS if every_k else (10,)
    x_ld, i_ld = lr.model(key, "ld", ks[-1], 10, False, None, ks)
    x_T, i_T = lr.model(key, T, ks[-1], 10, False, None, ks)
    worst = {}
    print()
    for K in ks:
        x, info = _solve(p, f32, K, False)
        assert info["iterations"] == K and not info["converged"] and info["compactions"] == 0
        assert info["checks"] == 2 + (K - 1) // 10 and info["rounds"] == 1 and info["width"] == p["A"].shape[1]
        assert all(word in info["plan"] for word in _plan_words(p)), info["plan"]
        _check_step(p, info)
        worst[K] = _check_x("%s K=%d" % (arm, K), x, i_T["snapshots"][K], i_ld["snapshots"][K], f32)
        if p.get("ic") and K == ks[-1]:     # (the model's intercept is the last iterate's)
            worst["c"] = _check_intercept("%s K=%d" % (arm, K), info, i_T, i_ld, f32)
    if every_k:     # once from a random nonzero x0
        n, l = p["A"].shape[1], p["b"].shape[1]
        x0 = lr.start(n, l, 0.1, f32)
        x_ld, i_ld = lr.model(key, "ld", 10, 10, False, 0.1)
        x_T, i_T = lr.model(key, T, 10, 10, False, 0.1)
        x, info = _solve(p, f32, 10, False, x0=x0)
        assert info["iterations"] == 10 and not info["converged"] and info["compactions"] == 0
        worst["x0"] = _check_x("%s K=10 x0" % arm, x, x_T, x_ld, f32)
        if p.get("ic"):
            worst["x0 c"] = _check_intercept("%s K=10 x0" % arm, info, i_T, i_ld, f32)
    assert all(v <= 1 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------ b, c
COUNTERS =("iterations", "kept_history", "compactions", "width", "kept", "checks", "rounds")


def _assert_loop(arm, case, certificate=True, converged=True):
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
    if converged:
        assert info["converged"] == i_ld["converged"]
    assert np.array_equal(info["kept_rows"], i_ld["kept_rows"])
    if p["ptr"] is not None:
        assert np.array_equal(info["kept_groups"], i_ld["kept_groups"])
    if p.get("tau") is not None:    # the sparse-group arm's second history, and its count of rows
        print("    rows %s; model %s" % (info["kept_row_history"], i_ld["kept_row_history"]))
        assert info["kept_row_history"] == i_ld["kept_row_history"] == lr.ROW_HISTORIES[name]
        assert all(r >= g for r, g in zip(info["kept_row_history"], info["kept_history"]))
        assert len(info["kept_row_history"]) == len(info["kept_history"])
        assert info["nonzero_rows"] == int(np.count_nonzero(np.any(x != 0, axis=1)))
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


@pytest.mark.parametrize("key", [("ic", 40, 200, 3, 0.5, False, None, None, "general"),
                                 ("sgl", 40, 200, 3, 0.5, False, gr.POOL_SMALL, 0.3)], ids=lambda k: k[0])
def test_maxit_zero_intercept_and_sparse_group(key):
    """maxit = 0 in the two later arms: x0 comes back byte for byte after one check, with its own certificate."""
    p = lr.problem(*key)
    n, l = p["A"].shape[1], p["b"].shape[1]
    x0 = lr.start(n, l, 1.0)
    _, i_ld = lr.model(key, "ld", 0, 10, True, 1.0)
    assert i_ld["compactions"] == 0 and i_ld["checks"] == 1 and i_ld["min_margin"] >= 1e-6
    assert np.array_equal(i_ld["kept_rows"], np.arange(n))      # (so far from the optimum nothing is proven)
    x, info = _solve(p, False, 0, True, x0=x0)
    assert x.tobytes() == x0.tobytes()
    for k in COUNTERS:
        assert info[k] == i_ld[k], k
    assert not info["converged"] and np.array_equal(info["kept_rows"], np.arange(n))
    if key[0] == "sgl":
        assert info["kept_row_history"] == [] and np.array_equal(info["kept_groups"], np.arange(p["gw"].size))
    _assert_certificate(p, x, info)


@pytest.mark.parametrize("shape", [(40, 130, 3, 0.1), (96, 512, 16, 0.5)], ids=lambda c: "%dx%dx%d@%g" % c)
def test_maxit_exhausted(shape):
    case = ("maxit=7 %dx%dx%d" % shape[:3], ("rows",) + shape, 7, 10, None, [])
    x, info = _assert_loop("c", case)
    assert info["iterations"] == 7 and not info["converged"] and info["checks"] == 2


@pytest.mark.parametrize("case", lr.BRANCH_CASES, ids=lambda c: c[0])
def test_branches(case):
    name, key, maxit, check_every, x0_scale, want = case
    p = lr.problem(*key)
    # with an intercept the certificate of x = 0 sums w r_c^2 and w r_c b separately, r_c = fl(b-bar - b): its
    # gap is rounding dust of either sign (glx.path's docstring says so), and so is `converged` at tol = 1e-30
    dust = want[-1:] == [0] and bool(p.get("ic"))
    x, info = _assert_loop("c", case, converged=not dust)
    if want[-1:] == [0]:        # kept == 0 from a warm start
        assert np.all(x == 0) and not np.any(np.signbit(x))
        assert info["kept"] == 0 and info["kept_rows"].size == 0 and info["width"] == 0
        bl = p["b"].astype(LD)
        if dust:
            # gap = sum r_c (r_c + b) = b-bar . sum_j r_c + sum r_c delta, |delta| <= eps |r_c| / 2, and the column
            # sums of r_c are the rounding of the means' own sums (m + 2 terms, over |b|); the two fp64 sums of
            # m l terms and compose's three operations on them come on top
            m, l = bl.shape
            bbar = np.mean(bl, axis=0)
            half = float(np.sum((bl - bbar) ** 2) / 2)
            bar = gr.gamma(m * l + m + 8, EPS64) * (float(np.max(np.abs(bbar)) * np.sum(np.abs(bl))) + 6.0 * half)
            print("    gap %.3e (bar %.3e), converged %s" % (info["gap"], bar, info["converged"]))
            assert abs(info["gap"]) <= bar and info["converged"] == (info["rel_gap"] <= TOL)
            assert np.max(np.abs(info["intercept"] - bbar)) <= gr.gamma(m + 2, EPS64) * float(np.max(np.mean(np.abs(bl), axis=0)))
        else:
            half = float(np.sum(bl ** 2) / 2)
            assert info["converged"] and info["gap"] == 0.0
        assert abs(info["primal"] - half) <= 33 * EPS64 * 2 * half      # (test_gpu_certificate's bar of ||r||^2)
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
    """name -> (A, sample weights or None, dtype, max_steps, may_warn[, sigma: the centred operator])."""
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
    # center_sum: lambda_max(A^T W P A), P = I - 1 w^T / sigma, the step of the problem with an intercept. A sixth
    # entry, sigma = the sum of the weights as rounded to the dtype (m without), marks them. Column offsets 5
    # times the columns' spread make the uncentred operator's top eigenvalue ~ 25 m times the centred one's.
    g = np.random.default_rng(43)
    off = g.standard_normal((40, 130)) + 5.0 * g.standard_normal(130)[None, :]
    w96, w64 = _quarter_zero(9, 96), _quarter_zero(10, 64)
    a32 = g.standard_normal((64, 320)) + 5.0 * g.standard_normal(320)[None, :]
    out.update({
        "centred, offsets 5x 40x130": (off, None, np.float64, 400, False, 40.0),
        "centred, weights with zeros 96x200": (g.standard_normal((96, 200)), w96, np.float64, 400, False,
                                               float(np.sum(w96))),
        "centred, weights with zeros m<n f32": (a32, w64, np.float32, 400, False,
                                                float(np.sum(w64.astype(np.float32), dtype=np.float64))),
    })
    return out


LANCZOS = ["flat top x^4 n=500", "linspace 600, 60 steps", "random 40x130", "random 64x1024", "random 64x1024 f32",
           "n=1", "n=3", "zero columns", "rank 1", "pair 1e-10 apart", "20 within 1e-6", "weights with zeros",
           "weights with zeros m<n f32", "centred, offsets 5x 40x130", "centred, weights with zeros 96x200",
           "centred, weights with zeros m<n f32"]


@functools.lru_cache(maxsize=None)
def _lanczos_case(name):
    return _lanczos_cases()[name]


@pytest.mark.parametrize("name", LANCZOS)
def test_lambda_max(name):
    import torch
    from glx.solver import _lambda_max
    case = _lanczos_case(name)
    A, w, dt, max_steps, may_warn = case[:5]
    sigma = case[5] if len(case) > 5 else None
    A = A.astype(dt)
    wd = None if w is None else torch.as_tensor(w.astype(dt), device="cuda")
    A64 = A.astype(np.float64)
    kw = {}
    if sigma is None:
        At = A64 if w is None else np.sqrt(w.astype(dt).astype(np.float64))[:, None] * A64
        want = float(np.linalg.eigvalsh(At.T @ At)[-1])
    else:       # the centred weighted Gram matrix A^T W P A, P = I - 1 w^T / sigma, in float64
        m = A64.shape[0]
        w1 = np.ones(m) if w is None else w.astype(dt).astype(np.float64)
        P = np.eye(m) - np.outer(np.ones(m), w1) / sigma
        gram = A64.T @ (w1[:, None] * (P @ A64))
        want = float(np.linalg.eigvalsh(0.5 * (gram + gram.T))[-1])
        kw["center_sum"] = sigma
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = float(_lambda_max(torch.as_tensor(A, device="cuda"), max_steps=max_steps, sample_weight=wd, **kw))
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
