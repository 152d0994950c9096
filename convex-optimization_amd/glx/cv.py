"""K-fold cross-validation over the mu path, on the caller's A.

A fold is a 0/1 vector of observation weights (``sample_weight`` of :func:`glx.solve_certified`): the
training problem of fold k is ``1/2 sum_j w_j [fold_j != k] ||(A x - b)_j||^2 + mu Omega(x)`` and its
validation loss ``1/2 sum_j w_j [fold_j = k] ||(A x - b)_j||^2 / sum_j w_j [fold_j = k]`` comes out of the
final certificate's own launch (``holdout_weight``). No row of A is copied and A is never written;
the K folds share the device copies of A and b and one workspace. The price is that held-out rows
are still streamed by both passes, 1/K of each (DESIGN.md "Sample weights and cross-validation").

The helpers :func:`fold_labels`, :func:`fold_weights` and :func:`aggregate` are host only.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .certificate import _np_dtype, _rows_of, check_sample_weight


def fold_labels(folds, m: int) -> Tuple[np.ndarray, int]:
    """``folds`` as m labels in 0 .. K - 1 and K. An int K puts row j into fold j mod K (deterministic:
    there is no RNG in the library; pass a shuffled label array for anything else). An array must hold
    m integer labels that are exactly 0 .. K - 1. ValueError for fewer than two folds, a fold without
    rows, a wrong length and labels that are not integers."""
    m = int(m)
    if isinstance(folds, (int, np.integer)) and not isinstance(folds, bool):
        K = int(folds)
        if K < 2:
            raise ValueError("folds: at least two folds are needed (got %d)" % K)
        if K > m:
            raise ValueError("folds: %d folds of %d rows leave a fold empty" % (K, m))
        return np.arange(m, dtype=np.int64) % K, K
    lab = np.asarray(folds.detach().cpu().numpy() if hasattr(folds, "detach") else folds)
    if lab.ndim != 1 or lab.size != m:
        raise ValueError("folds must be an int or one label per row of A (%d), got shape %s" % (m, tuple(lab.shape)))
    if not np.issubdtype(lab.dtype, np.integer):
        raise ValueError("fold labels must be integers")
    lab = lab.astype(np.int64)
    if lab.min() < 0:
        raise ValueError("fold labels must be >= 0")
    K = int(lab.max()) + 1
    if K < 2:
        raise ValueError("folds: the labels name only one fold")
    counts = np.bincount(lab, minlength=K)
    if np.any(counts == 0):
        raise ValueError("folds: fold %d has no rows (labels must be exactly 0 .. K - 1)" % int(np.argmin(counts)))
    return lab, K


def fold_weights(labels: np.ndarray, k: int, sample_weight: Optional[np.ndarray] = None,
                 dtype=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """The training and hold-out weights of fold k: ``sample_weight * [labels != k]`` and
    ``sample_weight * [labels == k]`` (``sample_weight`` None: ones), arrays of ``dtype``. ValueError
    where either side has no positive weight (the sample weights put all of a fold's mass to zero)."""
    lab = np.asarray(labels)
    base = np.ones(lab.size, dtype=dtype) if sample_weight is None else np.asarray(sample_weight, dtype=dtype)
    if base.shape != lab.shape:
        raise ValueError("sample_weight must have one entry per fold label")
    hold = np.where(lab == int(k), base, 0).astype(dtype)
    train = np.where(lab == int(k), 0, base).astype(dtype)
    if not np.any(train > 0):
        raise ValueError("fold %d: no training row has a positive weight" % int(k))
    if not np.any(hold > 0):
        raise ValueError("fold %d: no held-out row has a positive weight" % int(k))
    return np.ascontiguousarray(train), np.ascontiguousarray(hold)


def aggregate(fold_loss, mus: Sequence[float]) -> Dict[str, Any]:
    """The cross-validation curve from the K x n_mus validation losses: ``mean`` over folds, ``se`` =
    std(ddof = 1) / sqrt(K), ``best`` = the first index of the smallest mean, ``one_se`` = the
    smallest index (the largest mu: mus decrease) whose mean is at most mean[best] + se[best], and
    ``mu_best`` / ``mu_one_se``."""
    fl = np.asarray(fold_loss, dtype=np.float64)
    mus = [float(v) for v in mus]
    if fl.ndim != 2 or fl.shape[0] < 2 or fl.shape[1] != len(mus) or not mus:
        raise ValueError("fold_loss must be K x n_mus with K >= 2, one column per mu")
    K = fl.shape[0]
    mean = fl.mean(axis=0)
    se = fl.std(axis=0, ddof=1) / math.sqrt(K)
    best = int(np.argmin(mean))
    one_se = int(np.flatnonzero(mean <= mean[best] + se[best])[0])
    return {"mean": mean, "se": se, "best": best, "one_se": one_se, "mu_best": mus[best], "mu_one_se": mus[one_se]}


def check_cv_args(A, b, folds, mus, n_mus, mu_min_ratio, sample_weight, groups, weights, tol, maxit, check_every):
    """Every check :func:`cv_path` can make without a device: the shapes, tol, maxit, check_every, the
    groups and weights, the mu grid's own arguments, the sample weights, the fold labels and that
    every fold has training and held-out mass. Returns (gw, sw, labels, K, mus or None)."""
    from .screen import _check_args, _check_mus, mu_grid
    gw = _check_args(A, b, None, tol, maxit, check_every, groups, weights)
    sw = check_sample_weight(sample_weight, _rows_of(A), _np_dtype(A))
    if mus is not None:
        mus = _check_mus(mus)
    else:
        mu_grid(1.0, n_mus, mu_min_ratio)
    labels, K = fold_labels(folds, _rows_of(A))
    for k in range(K):
        fold_weights(labels, k, sw, _np_dtype(A))
    return gw, sw, labels, K, mus


def cv_path(A, b, folds=5, mus: Optional[Sequence[float]] = None, n_mus: int = 10, mu_min_ratio: float = 1e-2,
            sample_weight=None, groups=None, weights=None, tol: float = 1e-6, maxit: Optional[int] = None,
            screen: bool = True, check_every: int = 10, refit: bool = False,
            fit_intercept: bool = False, row_ratio=None) -> Dict[str, Any]:
    """K-fold cross-validation of :func:`glx.path` over mu.

    ``folds``: an int K (row j goes to fold j mod K) or m fold labels 0 .. K - 1 (:func:`fold_labels`).
    The mu grid is computed once on the full data: ``mus``, or ``n_mus`` values from
    ``glx.mu_max(A, b, sample_weight=...)`` down to ``mu_min_ratio`` of it. Each fold runs one
    warm-started :func:`glx.path` with the training weights ``sample_weight * [fold != k]`` and the
    hold-out weights ``sample_weight * [fold = k]`` (:func:`fold_weights`); ``groups`` / ``weights``,
    ``tol``, ``maxit``, ``screen`` and ``check_every`` are the solves'. ``fit_intercept`` is passed
    through: every fold then fits its own unpenalised intercept (the weighted mean differs from fold to
    fold, and no fold centres or copies A), the grid starts at ``glx.mu_max(..., fit_intercept=True)`` of
    the full data and a fold's validation loss is taken with its training intercept. ``row_ratio`` (the
    sparse-group penalty of :func:`glx.solve_certified`) is passed through as well; the grid then starts at
    ``glx.mu_max(..., row_ratio=...)``.

    Returns a dict: ``mus``, ``fold_loss`` (K x n_mus: each fold's ``holdout_loss``), ``mean``, ``se``
    (standard error over folds, ddof 1), ``best`` (index of the smallest mean), ``one_se`` (the
    largest mu whose mean is within one standard error of the best), ``mu_best``, ``mu_one_se``,
    ``info`` (per fold, the list of the path's info dicts), ``folds`` (K) and, with ``refit=True``,
    ``refit``: the full-data path's ``(mu, x, info)`` entry at ``mu_best`` (warm-started down the grid
    to it)."""
    from . import screen as _screen
    maxit = _screen.DEFAULT_MAXIT if maxit is None else maxit
    gw, sw, labels, K, mus = check_cv_args(A, b, folds, mus, n_mus, mu_min_ratio, sample_weight, groups, weights,
                                           tol, maxit, check_every)
    from .certificate import check_row_ratio
    tau = check_row_ratio(row_ratio, gw, bool(fit_intercept))
    dt = _np_dtype(A)
    prep = _screen._Prepared(A, b, screen, None, gw, sw, weighted=True, intercept=bool(fit_intercept), tau=tau)
    if mus is None:
        mus = _screen.mu_grid(_screen._top(prep, gw, sw), n_mus, mu_min_ratio)
    fold_loss = np.zeros((K, len(mus)), dtype=np.float64)
    infos: List[List[Dict[str, Any]]] = []
    for k in range(K):
        train, hold = fold_weights(labels, k, sw, dt)
        prep.set_weights(train)
        entries = _screen._run_path(prep, mus, tol, maxit, check_every, hold)
        fold_loss[k] = [e[2]["holdout_loss"] for e in entries]
        infos.append([e[2] for e in entries])
    out: Dict[str, Any] = {"mus": list(mus), "fold_loss": fold_loss, "folds": K, "info": infos}
    out.update(aggregate(fold_loss, mus))
    if refit:
        prep.set_weights(sw)
        out["refit"] = _screen._run_path(prep, mus[:out["best"] + 1], tol, maxit, check_every)[-1]
    return out


def format_table(cv: Dict[str, Any]) -> str:
    """The CV table of the driver: one line per mu with the mean, the standard error and a marker on
    the best and the one-standard-error choice."""
    lines = ["%-4s %-14s %-14s %-14s %s" % ("#", "mu", "mean", "se", "")]
    for i, mu in enumerate(cv["mus"]):
        mark = " ".join(t for t, on in (("best", i == cv["best"]), ("1-SE", i == cv["one_se"])) if on)
        lines.append("%-4d %-14.6e %-14.6e %-14.6e %s" % (i, mu, cv["mean"][i], cv["se"][i], mark))
    return "\n".join(lines)
