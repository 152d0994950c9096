"""NumPy statement of the primal ADMM iteration libglx runs (csrc/admm_primal.cpp), for the tests.

The reference (``code/gl_ADMM_primal.py:62, 78``) solves with the Cholesky factor of
``rho I + A^T A`` (n x n) at every iteration. The library restructures that, and this file restates
the restructured iteration term by term, in both of its forms:

* direct (``form=1``): ``Kn = (rho I + A^T A)^-1`` explicitly, once, in float64, then cast to A's
  dtype; ``y+ = Kn w``;
* Woodbury (``form=2``): ``K = (rho I + A A^T)^-1`` (m x m) likewise; ``v = (AATb - Az) + rho Ax``
  from the two products of the batched pass ``A @ [x | z]``, ``q = K v``, ``g = A^T q``,
  ``y+ = (w - g) / rho``;
* ``form=0`` resolves to Woodbury exactly when ``m^2 + m n < n^2``;
* ``w = (ATb - z) + rho x``, and the row step in the reference's evaluation order (``:47-51, 80-84``):
  ``p = x - (eta rho)((x - y+) - z / rho)``, ``x+ = (p max(||p_i|| - eta mu, 0)) / ((||p_i|| < thres)
  + ||p_i||)``, ``z+ = z - (tau rho)(x+ - y+)``, ``r = x+ - y+``, ``s = y+ - y``;
* the spectral norms of r and s (``LA.norm(., ord=2)``, ``:99-100``) as the square roots of the
  largest eigenvalues of the l x l Gram matrices, accumulated in float64.

``tests/test_admm_primal_cpu.py`` checks that this reproduces the reference's recorded runs
(``tests/golden/admm_primal_*.npz``); ``tests/test_gpu_admm_primal.py`` checks the GPU against the
same fixtures and against this file where options vary.
"""
from __future__ import annotations

import math

import numpy as np

from admm_ref import spectral_norm_gram

DEFAULT_OPTS = {"maxit": 100, "thres": 1e-3, "tau": (1 + math.sqrt(5)) * 0.5, "rho": 1e-2, "eta_0": 100,
                "converge_len": 10, "converge_thres": 1e-5, "step_type": "fixed", "form": 0}


def resolve_form(form: int, m: int, n: int) -> int:
    if form:
        return form
    return 2 if m * m + m * n < n * n else 1


def spd_inverse(M: np.ndarray) -> np.ndarray:
    L = np.linalg.cholesky(M)
    Li = np.linalg.solve(L, np.identity(M.shape[0]))
    return Li.T @ Li


def setup(A: np.ndarray, b: np.ndarray, rho: float, form: int):
    """(K, ATb, AATb) in A's dtype from float64: Kn (n x n) for form 1, K (m x m) for form 2."""
    a, bb = A.astype(np.float64), b.astype(np.float64)
    ATb = a.T @ bb
    if form == 2:
        K = spd_inverse(rho * np.identity(a.shape[0]) + a @ a.T)
        AATb = (a @ ATb).astype(A.dtype)
    else:
        K = spd_inverse(rho * np.identity(a.shape[1]) + a.T @ a)
        AATb = None
    return K.astype(A.dtype), ATb.astype(A.dtype), AATb


def step_eta(eta_0, step_type: str, k: int) -> float:
    if step_type == "fixed":
        return float(eta_0)
    if step_type == "diminishing":
        return float(eta_0) / math.sqrt(k)
    if step_type == "diminishing2":
        return float(eta_0) / k
    raise ValueError(step_type)


def row_step(yn, x, y, z, ATb, rho, tau, eta, mu, thres):
    """(x+, z+, r, s, w+) of one row step on y+ = yn, in x's dtype with the scalars rounded to it
    first (the kernel's rule; NEP 50's for Python floats)."""
    dt = x.dtype.type
    rho_, etarho, etamu, taurho, thres_ = dt(rho), dt(eta * rho), dt(eta * mu), dt(tau * rho), dt(thres)
    p = x - etarho * ((x - yn) - z / rho_)
    nr = np.sqrt(np.sum(p * p, axis=1, dtype=x.dtype)).reshape(-1, 1)
    xn = (p * np.clip(nr - etamu, a_min=0, a_max=None)) / ((nr < thres_).astype(x.dtype) + nr)
    r = xn - yn
    zn = z - taurho * r
    s = yn - y
    wn = (ATb - zn) + rho_ * xn
    return xn, zn, r, s, wn


def gl_admm_primal(x0, A, b, mu, opts=None):
    """Returns (x, k, out); out adds the per-iteration norms ``r_norm``, ``s_norm`` and ``form``."""
    o = {**DEFAULT_OPTS, **(opts or {})}
    rho, tau, thres = o["rho"], o["tau"], o["thres"]
    dt = A.dtype
    m, n = A.shape
    form = resolve_form(int(o["form"]), m, n)
    K, ATb, AATb = setup(A, b, rho, form)
    x = np.copy(x0).astype(dt)
    y, z = x.copy(), x.copy()
    rho_ = dt.type(rho)
    w = (ATb - z) + rho_ * x
    Ax = A @ x
    Az = A @ z if form == 2 else None
    f_hist, f_best_hist, rns, sns = [], [], [], []
    f_best = np.inf

    def objective(Ax, x):
        res = Ax - b
        return 0.5 * float(np.sum((res * res).astype(np.float64))) + mu * float(
            np.sum(np.sqrt(np.sum(x * x, axis=1, dtype=dt)).astype(np.float64)))

    f0 = objective(Ax, x)
    k = length = 0
    while k < o["maxit"]:
        k += 1
        eta = step_eta(o["eta_0"], o["step_type"], k)
        if form == 2:
            v = (AATb - Az) + rho_ * Ax
            q = K @ v
            g = A.T @ q
            yn = (w - g) / rho_
        else:
            yn = K @ w
        x, z, r, s, w = row_step(yn, x, y, z, ATb, rho, tau, eta, mu, thres)
        y = yn
        Ax = A @ x
        if form == 2:
            Az = A @ z
        f = objective(Ax, x)
        f_hist.append(f)
        f_best = min(f_best, f)
        f_best_hist.append(f_best)
        rn, sn = spectral_norm_gram(r), spectral_norm_gram(s)
        rns.append(rn)
        sns.append(sn)
        length = length + 1 if (rn < thres and sn < thres) else 0
        if length >= o["converge_len"]:
            break
    fval = f_hist[-1] if f_hist else f0
    return x, k, {"fval": fval, "f_hist": f_hist, "f_hist_best": f_best_hist, "r_norm": rns,
                  "s_norm": sns, "form": form}
