"""The loops of the three splitting solvers (csrc/admm.cpp, admm_primal.cpp, alm.cpp) in NumPy, as
the test reference of whole solves iterate by iterate (tests/test_split_loop_ref_cpu.py pins it,
tests/test_gpu_split_loops.py compares the GPU loops with it).

It restates the loops of admm_ref.py, admm_primal_ref.py and alm_dual_ref.py around their own
row_step and inner_step (imported, not copied) and differs from them in three ways:

  * the precomputed matrices are arguments: K for dual ADMM; (K, ATb, AATb) for primal ADMM, K being
    Kn (n x n) in the direct form and K (m x m) in Woodbury's; (K, Qn) for dual ALM. A GPU test
    hands in what glx.admm.inverse_factor, glx.admm_primal.setup and glx.alm.inner_matrix returned,
    so the setup is an input to both sides and only the loop is compared;
  * the working type is a parameter (np.longdouble, np.float64 or np.float32): every array the loop
    holds and every product is in it; the objective's two sums and the Gram matrices of the stop rule
    are accumulated in float64 (in longdouble for a longdouble run), as the kernels accumulate them;
  * `splits` sums every dense product over that many column blocks of the matrix in ascending order,
    as a K-split launch does. It serves to measure d(K) only.

Each run returns a dict: x, k, fval, f_hist, f_hist_best, r_norm, s_norm, length (the streak of the
stop rule after every iteration) and snapshots[it] = x after iteration it for it in `snap`. With
thres = 0 the iterates do not depend on maxit, so one run serves every shorter one.

All inputs are float64 arrays holding what the GPU is given (already rounded where it works in
float32). Imports nothing from glx.
"""
import functools
import math

import numpy as np

import admm_primal_ref
import admm_ref
import alm_dual_ref

LD = np.longdouble
TYPES = {"ld": LD, "f64": np.float64, "f32": np.float32}
TAU = (1 + math.sqrt(5)) * 0.5
DUAL_DEFAULTS = {"maxit": 100, "thres": 1e-3, "tau": TAU, "rho": 1e2, "converge_len": 20, "max_total_iters": 0}
PRIMAL_DEFAULTS = {"maxit": 100, "thres": 1e-3, "tau": TAU, "rho": 1e-2, "eta_0": 100.0, "converge_len": 10,
                   "step_type": "fixed", "max_total_iters": 0}
ALM_DEFAULTS = {"maxit": 100, "thres": 1e-3, "tau": TAU, "rho": 1e2, "converge_len": 20, "inner_iters": 500,
                "inner_step": 1e-2, "max_total_iters": 0}


def mm(M, X, splits=1):
    """M @ X as the sum, in ascending order, of `splits` products over column blocks of M."""
    if splits <= 1:
        return M @ X
    n = M.shape[1]
    edges = [n * i // splits for i in range(splits + 1)]
    acc = M[:, edges[0]:edges[1]] @ X[edges[0]:edges[1]]
    for i in range(1, splits):
        acc = acc + M[:, edges[i]:edges[i + 1]] @ X[edges[i]:edges[i + 1]]
    return acc


def _wide(T):
    return LD if T is LD else np.float64


def _objective(Ax, b, x, mu, T):
    """1/2 sum (Ax - b)^2 + mu sum_i ||x_i||: squares and row norms in T, both sums in the wide type."""
    W = _wide(T)
    res = Ax - b
    sq = float(np.sum((res * res).astype(W)))
    nr = float(np.sum(np.sqrt(np.sum(x * x, axis=1, dtype=T)).astype(W)))
    return 0.5 * sq + mu * nr


def _snorm(R, T):
    """The spectral norm of R from its l x l Gram matrix (accumulated in the wide type)."""
    r = R.astype(_wide(T))
    lam = float(np.linalg.eigvalsh((r.T @ r).astype(np.float64))[-1])
    return math.sqrt(max(lam, 0.0))


class _Log:
    """The host half of every loop: the objective's history, the best value and the stop rule."""

    def __init__(self, o, snap):
        self.thres, self.clen, self.snap = o["thres"], o["converge_len"], tuple(snap)
        self.f_hist, self.f_best_hist, self.rn, self.sn, self.lengths = [], [], [], [], []
        self.f_best, self.length, self.snapshots = math.inf, 0, {}

    def step(self, k, f, r, s, x, T):
        self.f_hist.append(f)
        self.f_best = f if f < self.f_best else self.f_best
        self.f_best_hist.append(self.f_best)
        rn, sn = _snorm(r, T), _snorm(s, T)
        self.rn.append(rn)
        self.sn.append(sn)
        self.length = self.length + 1 if (rn < self.thres and sn < self.thres) else 0
        self.lengths.append(self.length)
        if k in self.snap:
            self.snapshots[k] = x.copy()
        return self.length >= self.clen

    def result(self, x, k, f0):
        return {"x": x, "k": k, "fval": self.f_hist[-1] if self.f_hist else f0,
                "f_hist": np.asarray(self.f_hist, dtype=np.float64),
                "f_hist_best": np.asarray(self.f_best_hist, dtype=np.float64),
                "r_norm": np.asarray(self.rn), "s_norm": np.asarray(self.sn),
                "length": np.asarray(self.lengths, dtype=np.int64), "snapshots": self.snapshots}


def _maxit(o):
    return o["maxit"] if not o["max_total_iters"] else min(o["maxit"], o["max_total_iters"])


def dual_admm(x0, A, b, mu, K, opts=None, dtype=np.float64, splits=1, snap=()):
    """admm_solve (csrc/admm.cpp): v = (Ax - rho Au) - b, z = K v, g = A^T z, admm_ref.row_step,
    A @ [x+ | u+], s = Au - Au+."""
    o = {**DUAL_DEFAULTS, **(opts or {})}
    T = np.dtype(dtype).type
    rho, tau = o["rho"], o["tau"]
    A, b, K = (np.asarray(a, dtype=np.float64).astype(T) for a in (A, b, K))
    At = np.ascontiguousarray(A.T)
    x = np.asarray(x0, dtype=np.float64).astype(T)
    u = np.zeros_like(x)
    Ax, Au = mm(A, x, splits), mm(A, u, splits)
    f0 = _objective(Ax, b, x, mu, T)
    log = _Log(o, snap)
    k = 0
    while k < _maxit(o):
        k += 1
        v = (Ax - rho * Au) - b
        z = mm(K, v, splits)
        g = mm(At, z, splits)
        un, xn, r = admm_ref.row_step(x, g, rho, tau, mu)
        Axn, Aun = mm(A, xn, splits), mm(A, un, splits)
        s = Au - Aun
        x, u, Ax, Au = xn, un, Axn, Aun
        if log.step(k, _objective(Ax, b, x, mu, T), r, s, x, T):
            break
    return log.result(x, k, f0)


def primal_admm(x0, A, b, mu, K, ATb, AATb, form, opts=None, dtype=np.float64, splits=1, snap=()):
    """primal_solve (csrc/admm_primal.cpp) in the given form (1 direct: K is Kn, AATb unused;
    2 Woodbury): w = (ATb - z) + rho x, y+ = K w or (w - A^T K v) / rho with
    v = (AATb - Az) + rho Ax, then admm_primal_ref.row_step."""
    o = {**PRIMAL_DEFAULTS, **(opts or {})}
    T = np.dtype(dtype).type
    rho, tau, thres = o["rho"], o["tau"], o["thres"]
    A, b, K, ATb = (np.asarray(a, dtype=np.float64).astype(T) for a in (A, b, K, ATb))
    At = np.ascontiguousarray(A.T)
    if form == 2:
        AATb = np.asarray(AATb, dtype=np.float64).astype(T)
    x = np.asarray(x0, dtype=np.float64).astype(T)
    y, z = x.copy(), x.copy()
    rho_ = T(rho)
    w = (ATb - z) + rho_ * x
    Ax = mm(A, x, splits)
    Az = mm(A, z, splits) if form == 2 else None
    f0 = _objective(Ax, b, x, mu, T)
    log = _Log(o, snap)
    k = 0
    while k < _maxit(o):
        k += 1
        eta = admm_primal_ref.step_eta(o["eta_0"], o["step_type"], k)
        if form == 2:
            v = (AATb - Az) + rho_ * Ax
            q = mm(K, v, splits)
            g = mm(At, q, splits)
            yn = (w - g) / rho_
        else:
            yn = mm(K, w, splits)
        x, z, r, s, w = admm_primal_ref.row_step(yn, x, y, z, ATb, rho, tau, eta, mu, thres)
        y = yn
        Ax = mm(A, x, splits)
        if form == 2:
            Az = mm(A, z, splits)
        if log.step(k, _objective(Ax, b, x, mu, T), r, s, x, T):
            break
    return log.result(x, k, f0)


def dual_alm(x0, A, b, mu, K, Qn, opts=None, dtype=np.float64, splits=1, snap=()):
    """alm_solve (csrc/alm.cpp): J = rho (A^T K ((Ax - 0 Ax) - b) - x / rho), the inner loop of
    alm_dual_ref.inner_step from u = y = 0, z = K ((Ax - rho A u) - b), r = u + A^T z,
    x+ = x - (tau rho) r, A @ [x+ | u], s = Au_prev - Au."""
    o = {**ALM_DEFAULTS, **(opts or {})}
    T = np.dtype(dtype).type
    rho, tau, t = o["rho"], o["tau"], o["inner_step"]
    iters = int(o["inner_iters"])
    A, b, K, Qn = (np.asarray(a, dtype=np.float64).astype(T) for a in (A, b, K, Qn))
    At = np.ascontiguousarray(A.T)
    x = np.asarray(x0, dtype=np.float64).astype(T)
    Ax, Au = mm(A, x, splits), np.zeros_like(b)
    f0 = _objective(Ax, b, x, mu, T)
    log = _Log(o, snap)
    k = 0
    while k < _maxit(o):
        k += 1
        E = mm(K, (Ax - T(0) * Ax) - b, splits)
        J = rho * (mm(At, E, splits) - x / rho)
        u, y = np.zeros_like(J), np.zeros_like(J)
        for i in range(1, iters + 1):
            u, y = alm_dual_ref.inner_step(mm(Qn, y, splits), y, J, u, 2 / (i + 1), 2 / (i + 2) if i < iters else 0,
                                           t, mu)
        Au1 = mm(A, u, splits)
        z = mm(K, (Ax - rho * Au1) - b, splits)
        r = u + mm(At, z, splits)
        x = x - tau * rho * r
        Ax, Aun = mm(A, x, splits), mm(A, u, splits)
        s = Au - Aun
        Au = Aun
        if log.step(k, _objective(Ax, b, x, mu, T), r, s, x, T):
            break
    return log.result(x, k, f0)


# ------------------------------------------------------------------------------------------ bars
def distance(runs_T, run_ld, it):
    """d(K) and d_f(i), d_fbest(i) for i < K: the largest distance from the longdouble run of the
    working-type runs (splits 1, 2, 3), of x after iteration `it` and of the two histories."""
    xl = run_ld["snapshots"][it]
    dx = max(float(np.max(np.abs(r["snapshots"][it].astype(LD) - xl))) for r in runs_T)
    df = np.max([np.abs(r["f_hist"][:it] - run_ld["f_hist"][:it]) for r in runs_T], axis=0)
    db = np.max([np.abs(r["f_hist_best"][:it] - run_ld["f_hist_best"][:it]) for r in runs_T], axis=0)
    return dx, df, db


def bars(runs_T, run_ld, it, eps):
    """bar_x(K) = 16 d(K) + 4 eps max |x_LD| and the same form for every f_hist[i], f_hist_best[i]
    (loop_ref.x_bar's: d is what rounding alone does to this trajectory in NumPy's order of
    operations, 16 the project's margin for MFMA and split summation orders). Returns
    (bar_x, bar_f, bar_fbest, d / max |x_LD|)."""
    dx, df, db = distance(runs_T, run_ld, it)
    xmax = float(np.max(np.abs(run_ld["snapshots"][it])))
    bx = 16.0 * dx + 4.0 * eps * xmax
    bf = 16.0 * df + 4.0 * eps * np.abs(run_ld["f_hist"][:it])
    bb = 16.0 * db + 4.0 * eps * np.abs(run_ld["f_hist_best"][:it])
    return bx, bf, bb, dx / xmax


# ------------------------------------------------------------------------------------------ cases
GENERATED_SEED = 97006855   # oracle.numpy_ref.gen_data's seed for the shapes no golden covers


@functools.lru_cache(maxsize=None)
def instance(m, n, l):
    """(A, b, x0, mu) of a test shape, float64 and read-only: the golden instance where the dual ADMM
    goldens hold one (the three solvers' goldens share instances per shape), else generated."""
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "admm_index.json")) as fh:
        index = json.load(fh)
    name = "admm_dual_%dx%dx%d" % (m, n, l)
    if name in index:
        from test_admm_cpu import load_case
        _, _, A, b, x0, mu = load_case(name)
    else:
        from oracle import numpy_ref
        A, b, _, x0, mu = numpy_ref.gen_data(m, n, l, GENERATED_SEED)
    out = tuple(np.array(a, dtype=np.float64) for a in (A, b, x0))
    for a in out:
        a.setflags(write=False)
    return out + (float(mu),)


def numpy_setup(solver, A, b, rho, form=0):
    """The precomputed matrices from NumPy's own float64 setup (the restatements'), as a tuple in the
    order the loop takes them."""
    if solver == "dual":
        return (admm_ref.inverse_factor(A, rho),)
    if solver == "primal":
        return admm_primal_ref.setup(A, b, rho, form) + (form,)
    K = alm_dual_ref.inverse_factor(A, rho)
    return (K, alm_dual_ref.inner_matrix(A, K, rho))


LOOPS = {"dual": dual_admm, "primal": primal_admm, "alm": dual_alm}


def run(solver, shape, mats, opts, dtype, splits=1, snap=()):
    """LOOPS[solver] on instance(*shape); dtype "ld", "f64" or "f32" (the instance rounded to float32
    first, as a float32 solve sees it)."""
    A, b, x0, mu = instance(*shape)
    if dtype == "f32":
        A, b, x0 = (a.astype(np.float32).astype(np.float64) for a in (A, b, x0))
    return LOOPS[solver](x0, A, b, mu, *mats, opts=opts, dtype=TYPES[dtype], splits=splits, snap=snap)


# The stop-rule cases (thres, converge_len = 3): the streak becomes positive, resets and later
# reaches 3 at iteration k; margin = the least |norm / thres - 1| over every r_norm and s_norm up to
# k. Found with the float64 model and NumPy's setup, pinned in tests/test_split_loop_ref_cpu.py.
# (solver, shape, form, extra opts, thres, k, margin at least)
STOP_CASES = [
    ("dual", (100, 130, 3), 0, {}, 8.239e-5, 22, 9.9e-3),
    ("dual", (128, 256, 32), 0, {}, 2.19e-4, 34, 8.5e-2),
    ("primal", (128, 256, 32), 1, {}, 2400.0, 5, 0.117),
    ("primal", (128, 256, 32), 2, {}, 2400.0, 5, 0.117),
    # s_norm is not monotone here: 0.240, 0.178, 0.307, 0.329, 0.157, 0.093, 0.057
    ("alm", (64, 128, 16), 0, {"inner_iters": 7}, 0.205, 7, 0.13),
]
