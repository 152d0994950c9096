"""The loops of the three splitting solvers on the GPU against tests/split_loop_ref.py, iterate by
iterate: dual ADMM (glx.admm), primal ADMM in both forms (glx.admm_primal) and dual ALM (glx.alm).

The whole-solve tests of tests/test_gpu_admm.py, test_gpu_admm_primal.py and test_gpu_alm_dual.py hold
f_hist to 1e-8 and x to 1e-6 of the goldens, where the solvers measure 1e-13; this module holds every
iterate to what rounding does to it. The precomputed matrices (K; K, ATb, AATb; K, Qn) are computed
once on the GPU by the solvers' own setup functions and handed to the model as well, so only the loop
is compared. All arms run with thres = 0 unless they test the stop rule: only maxit stops them.

Bars, from the model alone (split_loop_ref.bars, the form of loop_ref.x_bar):
  bar_x(K)  = 16 d(K) + 4 eps_T max |x_LD(K)|
  bar_f(i)  = 16 d_f(i) + 4 eps_T |f_LD(i)|, likewise for f_hist_best
with d the largest distance from the longdouble run of the model's runs in T with every dense product
summed over 1, 2 and 3 column blocks: what rounding and the order of a K-split sum do to this
trajectory in NumPy. 16 is the project's margin for the MFMA and split summation orders of the
kernels. A loop mutation (a dropped slab, a wrong offset, a missing copy-back, an unconditional
f_best) sits many orders above these bars.

1. Trajectories: x, f_hist and f_hist_best after K = 1, 2, 3, 10, 25 iterations (dual ADMM's x
   ping-pongs between two buffers: K = 1, 2, 3 end on either side and take the final copy-back or
   not). ALM: inner_iters 1, 2, 7, 50 by K = 1, 2, 3, 8, the default 500 at K = 1, 2, and one inner
   step up to K = 30, past three rises of the objective (f_hist_best leaves f_hist only there).
2. Forced splits: GLX_AX_S = GLX_AXB_S = GLX_ATR_S = 2, then 3; the describe string must show that S
   for every product. The S > 1 arms of the glue kernels, launch_sum_partials on K, the P + S ml
   offset and the direct primal form's slabs of Kn w run here inside whole solves.
3. The stop rule: split_loop_ref.STOP_CASES (thres, converge_len = 3), where the model's streak
   becomes positive, resets and later reaches 3. The GPU's k is the model's and f_hist has that
   length; every norm of the model is at least 1e-3 from thres and the float64 and longdouble models
   agree within 1e-9, so no decision is a tie.
4. maxit = 0 returns x0's bits and its objective; max_total_iters below maxit stops there.

Measured on an MI355X, worst error / bar over the arms of a family (x, then f_hist and f_hist_best;
the module prints every arm's at teardown, pytest -s), and the model's d(K) / max |x_LD| over the
family's arms and K (from the CPU alone):
  dual ADMM fp64          x 0.082  f 0.58 (the m > n shape; <= 0.19 elsewhere)   d 2.9e-16 .. 2.8e-12
  dual ADMM fp32          x 0.084  f 0.29                                        d 1.4e-7 .. 1.9e-6
  primal ADMM fp64        x 0.11   f 0.27                                        d 2.5e-16 .. 2.2e-11
  primal ADMM fp32        x 0.060  f 0.14                                        d 1.7e-7 .. 1.7e-6
  dual ALM                x 0.073  f 0.17                                        d 5.8e-16 .. 9.6e-13
  forced S = 2, 3  dual   x 0.085  f 0.21     primal direct x 0.11 f 0.21
                   Woodbury x 0.056 f 0.098   ALM x 0.064 f 0.44
  stop rule (x at the stop)  0.052            maxit = 0 fval 0.23
None is above 1: no arm leaves the model, and no bug was found.

Mutations of the library (scratch builds, not committed), each run against this module and
tests/test_gpu_split_glue.py ("new") and against tests/test_gpu_admm.py, test_gpu_admm_primal.py and
test_gpu_alm_dual.py as they were ("old"); failed tests of each:
  slab_sum skipping slab 0 when S > 1      new 162   old 175
  P + S ml written P + ml, k_admm_fin      new 38    old 4      (k_admm_primal_fin: new 36, old 3)
  s = au - Au[idx]                         new 40    old 0      (test_admm_fin alone: the solvers read only ||s||)
  k_alm_j without / rho                    new 34    old 21
  rho for tau rho in the ALM x update      new 14    old 20
  launch_sum_partials skipped, SK > 1      new 4     old 0      (each solver; test_forced_splits)
  no final copy-back of x (dual ADMM)      new 11    old 2
  length never reset                       new 2, 2, 1 (dual, primal, ALM)   old 0   (test_stop_rule_...)
  f_best = f_now                           new 2, 8, 1 (dual, primal, ALM)   old 4, 19, 12
    (ALM: test_dual_alm_trajectory_past_a_rise alone; the K <= 8 arms never see f rise)
"""
import functools
import json

import numpy as np
import pytest

import split_loop_ref as sl

pytestmark = pytest.mark.gpu

MEASURED = {}
DREL = {}
EPS = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
KS = (1, 2, 3, 10, 25)
ALM_KS = (1, 2, 3, 8)
_MATS = {}


def _note(key, ratio):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nworst error / bar:", json.dumps({k: round(v, 4) for k, v in sorted(MEASURED.items())}))
        print("d(K) / max |x_LD|, (min, max):",
              json.dumps({k: ["%.1e" % min(v), "%.1e" % max(v)] for k, v in sorted(DREL.items())}))


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _arrays(shape, dtype):
    A, b, x0, mu = sl.instance(*shape)
    if dtype == "f32":
        return A.astype(np.float32), b.astype(np.float32), x0.astype(np.float32), mu
    return A, b, x0, mu


def _form(solver, shape, dtype, form):
    if solver != "primal":
        return 0
    from glx import _lib, admm_primal
    o = admm_primal.make_opts({"form": form})
    return admm_primal.resolved_form(_lib.GLX_F64 if dtype == "f64" else _lib.GLX_F32, *shape, o)


def _mats(solver, shape, dtype, rho, form):
    """The solver's own setup on the GPU, once per key, as float64 host arrays in the model's order."""
    key = (solver, shape, dtype, float(rho), form)
    if key not in _MATS:
        torch = _torch()
        from glx import admm, admm_primal, alm
        A, b, _, _ = _arrays(shape, dtype)
        Ad, bd = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
        host = lambda t: None if t is None else t.cpu().numpy().astype(np.float64)
        if solver == "dual":
            mats = (host(admm.inverse_factor(Ad, rho)),)
        elif solver == "primal":
            mats = tuple(host(t) for t in admm_primal.setup(Ad, bd, rho, form)) + (form,)
        else:
            K = admm.inverse_factor(Ad, rho)
            mats = (host(K), host(alm.inner_matrix(Ad, K, rho)))
        _MATS[key] = mats
    return key


@functools.lru_cache(maxsize=None)
def _model(key, opts, dtype, splits, maxit, snap):
    solver, shape = key[0], key[1]
    return sl.run(solver, shape, _MATS[key], {**dict(opts), "maxit": maxit}, dtype, splits=splits, snap=snap)


def _solve(solver, shape, dtype, opts):
    from glx import admm, admm_primal, alm
    A, b, x0, mu = _arrays(shape, dtype)
    mod = {"dual": admm, "primal": admm_primal, "alm": alm}[solver]
    return mod.solve(x0, A, b, mu, dict(opts))


def _default_rho(solver):
    return sl.PRIMAL_DEFAULTS["rho"] if solver == "primal" else 1e2


def _trajectory(tag, solver, shape, dtype="f64", opts=None, form=0, ks=KS, gpu_opts=None):
    """The GPU's x, f_hist and f_hist_best after each K of `ks` against the longdouble model's."""
    opts = {**(opts or {}), "thres": 0.0}
    form = _form(solver, shape, dtype, form)
    key = _mats(solver, shape, dtype, opts.get("rho", _default_rho(solver)), form)
    okey, top, snap = tuple(sorted(opts.items())), max(ks), tuple(ks)
    ld = _model(key, okey, "ld", 1, top, snap)
    runs = [_model(key, okey, dtype, S, top, snap) for S in (1, 2, 3)]
    worst = []
    for K in ks:
        bx, bf, bb, drel = sl.bars(runs, ld, K, EPS[dtype])
        DREL.setdefault(tag, []).append(drel)
        g = {**opts, "maxit": K, **(gpu_opts or {})}
        if solver == "primal":
            g["form"] = form
        x, k, out = _solve(solver, shape, dtype, g)
        assert k == K and len(out["f_hist"]) == K and len(out["f_hist_best"]) == K
        assert float(out["fval"]) == float(out["f_hist"][-1])
        ex = float(np.max(np.abs(x.astype(sl.LD) - ld["snapshots"][K]))) / bx
        ef = float(np.max(np.abs(np.asarray(out["f_hist"]) - ld["f_hist"][:K]) / bf))
        eb = float(np.max(np.abs(np.asarray(out["f_hist_best"]) - ld["f_hist_best"][:K]) / bb))
        print("%s K=%d: x err/bar %.3g, f_hist %.3g, f_hist_best %.3g, d(K)/max|x| %.2e" % (tag, K, ex, ef, eb, drel))
        worst.append((K, ex, ef, eb))
        _note(tag + " x", ex)
        _note(tag + " f", max(ef, eb))
    bad = [w for w in worst if max(w[1:]) > 1]
    assert not bad, (tag, bad)
    return out


# ---------------------------------------------------------------------------------------------
# 1. trajectories
# ---------------------------------------------------------------------------------------------
DUAL_SHAPES = [(100, 130, 3), (64, 128, 16), (128, 256, 32), (192, 128, 16)]


@pytest.mark.parametrize("shape", DUAL_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_dual_admm_trajectory(shape):
    """(100, 130, 3): the row kernel and VALU products; the others fuse the row step into A^T z
    (fused = 1, the default) and run it as the panel row kernel (fused = 2): the same bits."""
    from glx import _lib
    tag = "dual %dx%dx%d" % shape
    out = _trajectory(tag, "dual", shape)
    fuses = "projection=fused" in _lib.admm_describe(_lib.GLX_F64, *shape)
    assert fuses == (shape != (100, 130, 3)) and out["glx"]["fused"] == fuses
    if fuses:
        o2 = _trajectory(tag + " fused=2", "dual", shape, gpu_opts={"fused": 2})
        assert not o2["glx"]["fused"] and o2["f_hist"] == out["f_hist"]


@pytest.mark.parametrize("shape", [s for s in DUAL_SHAPES if s[0] < s[1]], ids=lambda s: "%dx%dx%d" % s)
def test_dual_admm_trajectory_f32(shape):
    _trajectory("dual f32 %dx%dx%d" % shape, "dual", shape, dtype="f32")


PRIMAL_ARMS = [((100, 130, 3), 0, {}), ((128, 256, 32), 1, {}), ((128, 256, 32), 2, {}), ((192, 128, 16), 1, {}),
               ((64, 128, 16), 0, {"step_type": "fixed"}), ((64, 128, 16), 0, {"step_type": "diminishing"}),
               ((64, 128, 16), 0, {"step_type": "diminishing2"}), ((64, 128, 16), 0, {"rho": 5e-2}),
               ((64, 128, 16), 0, {"tau": 1.0}), ((64, 128, 16), 0, {"eta_0": 50.0})]


def _arm_id(arm):
    shape, form, opts = arm
    return "%dx%dx%d-form%d%s" % (shape + (form,) + ("".join("-%s=%s" % kv for kv in sorted(opts.items())),))


@pytest.mark.parametrize("arm", PRIMAL_ARMS, ids=_arm_id)
def test_primal_admm_trajectory(arm):
    shape, form, opts = arm
    out = _trajectory("primal " + _arm_id(arm), "primal", shape, opts=opts, form=form)
    want = {0: None, 1: "direct", 2: "Woodbury"}[form]
    assert want is None or out["glx"]["form"] == want


def test_primal_admm_trajectory_f32():
    _trajectory("primal f32 192x128x16-form1", "primal", (192, 128, 16), dtype="f32", form=1)


@pytest.mark.parametrize("inner", [1, 2, 7, 50])
@pytest.mark.parametrize("shape", [(100, 130, 3), (64, 128, 16)], ids=lambda s: "%dx%dx%d" % s)
def test_dual_alm_trajectory(shape, inner):
    tag = "alm %dx%dx%d inner=%d" % (shape + (inner,))
    out = _trajectory(tag, "alm", shape, opts={"inner_iters": inner}, ks=ALM_KS)
    assert out["glx"]["inner_steps"] == inner * ALM_KS[-1]
    o2 = _trajectory(tag + " fused=2", "alm", shape, opts={"inner_iters": inner}, ks=ALM_KS, gpu_opts={"fused": 2})
    assert not o2["glx"]["fused"]


def test_dual_alm_trajectory_past_a_rise():
    """With one inner step the objective rises at iterations 25, 27 and 29 (by 2e-6 relative, the
    model's own f_hist asserted below): f_hist_best leaves f_hist, which it never does within the
    K <= 8 of the arms above."""
    out = _trajectory("alm 100x130x3 inner=1 K=30", "alm", (100, 130, 3), opts={"inner_iters": 1}, ks=(30,))
    fh, fb = np.asarray(out["f_hist"]), np.asarray(out["f_hist_best"])
    rises = np.nonzero(np.diff(fh) > 0)[0] + 2
    assert list(rises) == [25, 27, 29] and np.all(fb[rises - 1] < fh[rises - 1])


def test_dual_alm_trajectory_default_inner_loop():
    _trajectory("alm 100x130x3 inner=500", "alm", (100, 130, 3), ks=(1, 2))


# ---------------------------------------------------------------------------------------------
# 2. forced splits
# ---------------------------------------------------------------------------------------------
SPLIT_FIELDS = {"dual": ("K v=", "A [x|u]=", "A^T z="),
                "primal1": ("Kn w=", "A x="),
                "primal2": ("K v=", "A^T q=", "A [x|z]="),
                "alm": ("K v=", "A u=", "A [x|u]=", "A^T z=", "Qn y=")}


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("shape", [(100, 130, 3), (128, 256, 32)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("which", ["dual", "primal1", "primal2", "alm"])
def test_forced_splits(which, shape, S, monkeypatch):
    """Every dense product split S ways ((128, 256, 32) is the smallest MFMA shape at which the
    describe string shows the forced S for all of them, K's 128 x 128 included)."""
    from glx import _lib, admm_primal, alm
    for knob in ("GLX_AX_S", "GLX_AXB_S", "GLX_ATR_S"):
        monkeypatch.setenv(knob, str(S))
    solver = which.rstrip("12")
    form = int(which[-1]) if solver == "primal" else 0
    if solver == "dual":
        d = _lib.admm_describe(_lib.GLX_F64, *shape)
    elif solver == "primal":
        d = _lib.admm_primal_describe(_lib.GLX_F64, *shape, admm_primal.make_opts({"form": form}))
    else:
        d = _lib.alm_describe(_lib.GLX_F64, *shape, alm.make_opts({}))
    for field in SPLIT_FIELDS[which]:
        assert d.split(field)[1].split(";")[0].endswith("S=%d" % S), (field, d)
    opts = {"inner_iters": 7} if solver == "alm" else {}
    out = _trajectory("S=%d %s %dx%dx%d" % ((S, which) + shape), solver, shape, opts=opts, form=form,
                      ks=ALM_KS if solver == "alm" else (1, 2, 3, 10))
    assert out["glx"]["plan"] == d


# ---------------------------------------------------------------------------------------------
# 3. the stop rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sl.STOP_CASES, ids=["%s-%dx%dx%d-form%d" % ((c[0],) + c[1] + (c[2],))
                                                      for c in sl.STOP_CASES])
def test_stop_rule_passes_through_a_reset(case):
    solver, shape, form, extra, thres, k_pinned, _ = case
    opts = {**extra, "thres": thres, "converge_len": 3}
    key = _mats(solver, shape, "f64", _default_rho(solver), form)
    okey = tuple(sorted(opts.items()))
    m64, mld = _model(key, okey, "f64", 1, 60, ()), _model(key, okey, "ld", 1, 60, ())
    L, k = m64["length"], m64["k"]
    assert k == k_pinned and np.array_equal(mld["length"], L) and L[-1] == 3
    first = int(np.argmax(L > 0))
    assert L[first] > 0 and np.any(L[first + 1:k - 3] == 0), L
    norms = np.concatenate([m64["r_norm"], m64["s_norm"]])
    margin = float(np.min(np.abs(norms / thres - 1)))
    rel = lambda a, c: float(np.max(np.abs(a - c) / np.abs(c)))
    agree = max(rel(m64["r_norm"], mld["r_norm"]), rel(m64["s_norm"], mld["s_norm"]))
    print(solver, shape, form, "k", k, "margin %.3g" % margin, "f64 vs longdouble norms %.2e" % agree)
    assert margin >= 1e-3 and agree <= 1e-9
    g = {**opts, "maxit": 60}
    if solver == "primal":
        g["form"] = form
    x, kg, out = _solve(solver, shape, "f64", g)
    assert kg == k and len(out["f_hist"]) == k and len(out["f_hist_best"]) == k
    # the iterates it stopped on are the model's (the primal row step takes thres as its zero test)
    d = float(np.max(np.abs(m64["x"].astype(sl.LD) - mld["x"])))
    bar = 16.0 * d + 4.0 * EPS["f64"] * float(np.max(np.abs(mld["x"])))
    ex = float(np.max(np.abs(x.astype(sl.LD) - mld["x"]))) / bar
    print("  x err/bar %.3g" % ex)
    _note("stop %s %dx%dx%d x" % ((solver,) + shape), ex)
    assert ex <= 1


# ---------------------------------------------------------------------------------------------
# 4. maxit = 0 and max_total_iters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["dual", "primal1", "primal2", "alm"])
def test_maxit_zero_and_max_total_iters(which):
    shape = (128, 256, 32)
    solver = which.rstrip("12")
    form = int(which[-1]) if solver == "primal" else 0
    opts = {"thres": 0.0, **({"inner_iters": 7} if solver == "alm" else {})}
    key = _mats(solver, shape, "f64", _default_rho(solver), form)
    okey = tuple(sorted(opts.items()))
    A, b, x0, mu = _arrays(shape, "f64")
    g = dict(opts)
    if solver == "primal":
        g["form"] = form
    x, k, out = _solve(solver, shape, "f64", {**g, "maxit": 0})
    assert k == 0 and out["f_hist"] == [] and out["f_hist_best"] == []
    assert np.array_equal(x.view(np.uint64), x0.view(np.uint64))
    ld = _model(key, okey, "ld", 1, 0, ())
    d = max(abs(_model(key, okey, "f64", S, 0, ())["fval"] - ld["fval"]) for S in (1, 2, 3))
    bar = 16.0 * d + 4.0 * EPS["f64"] * abs(ld["fval"])
    _note("maxit=0 fval " + which, abs(float(out["fval"]) - ld["fval"]) / bar)
    assert abs(float(out["fval"]) - ld["fval"]) <= bar
    # max_total_iters below maxit stops there, on the iterate of maxit = 2
    x2, k2, o2 = _solve(solver, shape, "f64", {**g, "maxit": 9, "max_total_iters": 2})
    x3, k3, o3 = _solve(solver, shape, "f64", {**g, "maxit": 2})
    assert k2 == 2 and k3 == 2 and len(o2["f_hist"]) == 2
    assert np.array_equal(x2, x3) and o2["f_hist"] == o3["f_hist"]
