"""glx — MI355X-native group-lasso first-order solvers.

Public surface:
  * ``solve(name, x0, A, b, mu_0, opts)`` — the reference's ``gl_<method>`` contract
    (also re-exported as the drop-in modules ``gl_ProxGD_primal`` etc. next to this package);
  * ``Session`` — the same solver split into steps (benchmarks);
  * ``kernels`` — single HIP kernels (residual, gradient, prox);
  * ``admm`` — the dual ADMM solver ``gl_Admm_dual`` (``admm.solve``; drop-in module ``gl_ADMM_dual``);
  * ``admm_primal`` — the primal ADMM solver ``gl_Admm_primal`` (``admm_primal.solve``; drop-in module
    ``gl_ADMM_primal``);
  * ``alm`` — the dual ALM solver ``gl_Alm_dual`` (``alm.solve``; drop-in module ``gl_ALM_dual``);
  * ``certificate(x, A, b, mu)`` — the duality gap and KKT violation of any iterate, and
    ``mu_max(A, b)``, the smallest mu at which x = 0 is optimal (``glx/certificate.py``; the name
    ``glx.certificate`` is the function, so its module's helpers are reached with
    ``from glx.certificate import compose, record``);
  * ``solve_certified(A, b, mu)`` — a solve to a stated relative duality gap with gap-safe screening,
    and ``path(A, b)`` — the same over a decreasing sequence of mu, warm-started (``glx/screen.py``);
  * ``groups=`` / ``weights=`` on ``certificate``, ``mu_max``, ``solve_certified`` and ``path`` — the
    classical group lasso over contiguous feature groups with weights, and ``group_order(labels)``,
    the host-only helper that sorts arbitrary labels into such groups;
  * ``sample_weight=`` on the same four (and ``holdout_weight=`` on the two solves) — observation
    weights on the caller's A: weighted least squares, row subsets as 0/1 vectors, case weights; and
    ``cv_path(A, b, folds=5)`` — K-fold cross-validation over the mu path built on them (``glx/cv.py``);
  * ``dist`` — row sharding + RCCL communicator.
"""
from ._lib import LIB_PATH, GlxError, lib  # noqa: F401
from .solver import Session, solve  # noqa: F401
from .certificate import certificate, group_order, mu_max  # noqa: F401
from .screen import path, solve_certified  # noqa: F401
from .cv import cv_path  # noqa: F401

__all__ = ["solve", "Session", "lib", "LIB_PATH", "GlxError", "certificate", "mu_max",
           "solve_certified", "path", "group_order", "cv_path"]
