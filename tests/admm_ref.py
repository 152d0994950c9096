"""NumPy statement of the dual ADMM iteration libglx runs (csrc/admm.cpp), for the tests.

The reference (``code/gl_ADMM_dual.py:61-93``) solves with the Cholesky factor of
``I + rho A A^T`` at every iteration and multiplies ``A @ (x - rho u)``. The library restructures
that, and this file restates the restructured iteration term by term:

* ``K = (I + rho A A^T)^-1`` explicitly, once, in float64, then cast to A's dtype; ``z = K v``;
* ``v = (Ax - rho Au) - b`` from the two products of the batched pass ``A @ [x | u]``;
* the row step in the reference's evaluation order (``:44-46, 64-67``):
  ``w = x / rho - g``, ``u+ = (mu w) / max(||w_i||, mu)``, ``r = u+ + g``, ``x+ = x - (tau rho) r``;
* ``s = Au - Au+`` (the reference's ``A @ (u_k - u)``, ``:68``);
* the spectral norms of r and s (``LA.norm(., ord=2)``, ``:85-86``) as the square roots of the
  largest eigenvalues of the l x l Gram matrices ``r^T r`` and ``s^T s``, accumulated in float64.

``tests/test_admm_cpu.py`` checks that this reproduces the reference's recorded runs
(``tests/golden/admm_dual_*.npz``); ``tests/test_gpu_admm.py`` checks the GPU against the same
fixtures.
"""
from __future__ import annotations

import math

import numpy as np

DEFAULT_OPTS = {"maxit": 100, "thres": 1e-3, "tau": (1 + math.sqrt(5)) * 0.5, "rho": 1e2,
                "converge_len": 20}


def inverse_factor(A: np.ndarray, rho: float) -> np.ndarray:
    a = A.astype(np.float64)
    m = a.shape[0]
    L = np.linalg.cholesky(np.identity(m) + rho * (a @ a.T))
    Li = np.linalg.solve(L, np.identity(m))
    return (Li.T @ Li).astype(A.dtype)


def row_step(x: np.ndarray, g: np.ndarray, rho: float, tau: float, mu: float):
    """(u+, x+, r) of one row step, in x's dtype with NEP 50 weak scalars."""
    w = x / rho - g
    nrm = np.sqrt(np.sum(w * w, axis=1, dtype=x.dtype)).reshape(-1, 1)
    u = mu * w / np.clip(nrm, a_min=mu, a_max=None)
    r = u + g
    xn = x - tau * rho * r
    return u, xn, r


def spectral_norm_gram(R: np.ndarray) -> float:
    r = R.astype(np.float64)
    lam = float(np.linalg.eigvalsh(r.T @ r)[-1])
    return math.sqrt(max(lam, 0.0))


def gl_admm_dual(x0, A, b, mu, opts=None):
    """Returns (x, k, out); out adds the per-iteration norms ``r_norm`` and ``s_norm``."""
    o = {**DEFAULT_OPTS, **(opts or {})}
    rho, tau, thres = o["rho"], o["tau"], o["thres"]
    dt = A.dtype
    K = inverse_factor(A, rho)
    x = np.copy(x0).astype(dt)
    u = np.zeros_like(x)
    Ax, Au = A @ x, A @ u
    f_hist, f_best_hist, rns, sns = [], [], [], []
    f_best = np.inf
    k = length = 0
    while k < o["maxit"]:
        k += 1
        v = (Ax - rho * Au) - b
        z = K @ v
        g = A.T @ z
        un, xn, r = row_step(x, g, rho, tau, mu)
        Axn, Aun = A @ xn, A @ un
        s = Au - Aun
        x, u, Ax, Au = xn, un, Axn, Aun
        res = Ax - b
        f = 0.5 * float(np.sum((res * res).astype(np.float64))) + mu * float(
            np.sum(np.sqrt(np.sum(x * x, axis=1, dtype=dt)).astype(np.float64)))
        f_hist.append(f)
        f_best = min(f_best, f)
        f_best_hist.append(f_best)
        rn, sn = spectral_norm_gram(r), spectral_norm_gram(s)
        rns.append(rn)
        sns.append(sn)
        length = length + 1 if (rn < thres and sn < thres) else 0
        if length >= o["converge_len"]:
            break
    fval = f_hist[-1] if f_hist else None
    return x, k, {"fval": fval, "f_hist": f_hist, "f_hist_best": f_best_hist, "r_norm": rns,
                  "s_norm": sns}
