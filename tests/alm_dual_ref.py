"""NumPy float64 statement of the dual ALM iteration libglx runs (csrc/alm.cpp), for the tests.

The reference (``code/gl_ALM_dual.py:10-63, 116-148``) rebuilds ``T = (I + rho A A^T)^-1``,
``F = rho T A``, ``G = I - A^T F``, ``Q = F^T F + rho G^T G`` and ``J`` at every outer iteration. The
library restructures that with two identities, and this file restates the restructured iteration
term by term (it imports nothing from glx):

* ``G = (I + rho A^T A)^-1`` (Woodbury) and ``G A^T = A^T T``, hence ``F^T F = rho G (I - G)`` and
  ``Q = rho G =: Qn``, built once: ``Qn = rho (I - A^T (rho K A))`` from ``K = T``, symmetrised;
* ``(I + rho A A^T) E = A x - b`` gives ``F^T (E + b) = rho (G - I) H``, hence ``J = rho H`` with
  ``H = A^T K (A x - b) - x / rho``;
* the inner step in the reference's evaluation order (``:45-47, 56-61``), the state carried being
  (u, y): ``w = y - t (Qn y + J)``, ``u+ = (mu w) / max(||w_i||, mu)``, ``v+ = u + (u+ - u) / gamma``,
  ``y+ = (1 - gamma+) u+ + gamma+ v+``;
* ``z = K ((Ax - rho Au) - b)``, ``r = u + A^T z``, ``x+ = x - (tau rho) r``, ``s = Au_prev - Au``;
* the spectral norms of r and s as the square roots of the largest eigenvalues of the l x l Gram
  matrices, as in ``tests/admm_ref.py``.

Options are accepted as in the solver: the reference's five keys, ``inner_iters`` (500),
``inner_step`` (1e-2) and ``max_total_iters``; other keys are ignored.
"""
from __future__ import annotations

import math

import numpy as np

DEFAULT_OPTS = {"maxit": 100, "thres": 1e-3, "tau": (1 + math.sqrt(5)) * 0.5, "rho": 1e2,
                "converge_len": 20}
BUILD_DEFAULTS = {"inner_iters": 500, "inner_step": 1e-2, "max_total_iters": 0}


def inverse_factor(A: np.ndarray, rho: float) -> np.ndarray:
    a = A.astype(np.float64)
    m = a.shape[0]
    L = np.linalg.cholesky(np.identity(m) + rho * (a @ a.T))
    Li = np.linalg.solve(L, np.identity(m))
    return Li.T @ Li


def inner_matrix(A: np.ndarray, K: np.ndarray, rho: float) -> np.ndarray:
    """Qn = rho (I + rho A^T A)^-1 from K by Woodbury, symmetrised (glx.alm.inner_matrix)."""
    F = rho * (K @ A)
    Q = rho * (np.identity(A.shape[1]) - A.T @ F)
    return 0.5 * (Q + Q.T)


def inner_step(P, y, J, u, gamma, gamma_next, t, mu):
    """(u+, y+) of one inner step on P = Qn y; y+ is None when gamma_next == 0."""
    w = y - t * (P + J)
    nrm = np.sqrt(np.sum(w * w, axis=1)).reshape(-1, 1)
    un = mu * w / np.clip(nrm, a_min=mu, a_max=None)
    vn = u + (un - u) / gamma
    yn = None if gamma_next == 0 else (1 - gamma_next) * un + gamma_next * vn
    return un, yn


def inner_loop(Qn, J, iters, t, mu):
    u = np.zeros_like(J)
    y = np.zeros_like(J)
    for i in range(1, iters + 1):
        u, y = inner_step(Qn @ y, y, J, u, 2 / (i + 1), 2 / (i + 2) if i < iters else 0, t, mu)
    return u


def spectral_norm_gram(R: np.ndarray) -> float:
    lam = float(np.linalg.eigvalsh(R.T @ R)[-1])
    return math.sqrt(max(lam, 0.0))


def objective(A, b, x, mu):
    res = A @ x - b
    return 0.5 * float(np.sum(res * res)) + mu * float(np.sum(np.sqrt(np.sum(x * x, axis=1))))


def gl_alm_dual(x0, A, b, mu, opts=None):
    """Returns (x, k, out); out adds the per-iteration norms ``r_norm`` and ``s_norm``."""
    o = {**DEFAULT_OPTS, **BUILD_DEFAULTS, **(opts or {})}
    rho, tau, thres = o["rho"], o["tau"], o["thres"]
    maxit = o["maxit"] if not o["max_total_iters"] else min(o["maxit"], o["max_total_iters"])
    A = A.astype(np.float64)
    K = inverse_factor(A, rho)
    Qn = inner_matrix(A, K, rho)
    x = np.copy(x0).astype(np.float64)
    Ax, Au = A @ x, np.zeros_like(b, dtype=np.float64)
    f_hist, f_best_hist, rns, sns = [], [], [], []
    f_best = np.inf
    k = length = 0
    while k < maxit:
        k += 1
        E = K @ (Ax - b)
        J = rho * (A.T @ E - x / rho)
        u = inner_loop(Qn, J, o["inner_iters"], o["inner_step"], mu)
        Aun = A @ u
        z = K @ ((Ax - rho * Aun) - b)
        r = u + A.T @ z
        x = x - tau * rho * r
        s = Au - Aun
        Ax, Au = A @ x, Aun
        f = objective(A, b, x, mu)
        f_hist.append(f)
        f_best = min(f_best, f)
        f_best_hist.append(f_best)
        rn, sn = spectral_norm_gram(r), spectral_norm_gram(s)
        rns.append(rn)
        sns.append(sn)
        length = length + 1 if (rn < thres and sn < thres) else 0
        if length >= o["converge_len"]:
            break
    fval = f_hist[-1] if f_hist else objective(A, b, x, mu)
    return x, k, {"fval": fval, "f_hist": f_hist, "f_hist_best": f_best_hist, "r_norm": rns,
                  "s_norm": sns}
