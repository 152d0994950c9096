"""ctypes binding of libglx.so (the C ABI in include/glx.h).

The library is built in-tree (``make -C convex-optimization_amd``) and is linked against
PyTorch's bundled HIP runtime; ``torch`` is imported before the library is loaded so that the
process holds exactly one HIP runtime and torch's device pointers / streams are native to it.
There is no fallback: if the library is missing, :func:`lib` raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_size_t, c_uint8, c_void_p

import torch  # noqa: F401  (must be loaded first: it owns the HIP runtime libglx binds to)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libglx.so")

GLX_F32, GLX_F64 = 0, 1
GLX_PROXGD, GLX_FPROXGD, GLX_SGD, GLX_GD, GLX_FGD = range(5)
STEP_TYPES = {"line_search": 0, "fixed": 1, "diminishing": 2, "diminishing2": 3}
METHODS = {"gl_ProxGD_primal": GLX_PROXGD, "gl_FProxGD_primal": GLX_FPROXGD,
           "gl_SGD_primal": GLX_SGD, "gl_GD_primal": GLX_GD, "gl_FGD_primal": GLX_FGD}
COMM_ID_BYTES = 128


class GlxOpts(ctypes.Structure):
    _fields_ = [("maxit", c_int32), ("thres", c_double), ("step_type", c_int32),
                ("alpha0", c_double), ("ftol", c_double), ("stable_len_threshold", c_int32),
                ("ls_coeff", c_double), ("ls_maxit", c_int32), ("delta", c_double),
                ("continuous_subgradient", c_int32), ("exact_objective", c_int32),
                ("profile", c_int32), ("max_total_iters", c_int64), ("ax_variant", c_int32),
                ("split_cand", c_int32), ("dc_window", c_int32), ("shard_rows", c_int32),
                ("shard_model", c_int32), ("reserved", c_int32 * 3)]


class GlxProblem(ctypes.Structure):
    _fields_ = [("dtype", c_int32), ("method", c_int32), ("m", c_int64), ("n", c_int64),
                ("l", c_int64), ("A", c_void_p), ("b", c_void_p), ("x", c_void_p),
                ("mu0", c_double), ("comm", c_void_p)]


class GlxResult(ctypes.Structure):
    _fields_ = [("iters", c_int64), ("fval", c_double), ("tt", c_double),
                ("f_hist", POINTER(c_double)), ("f_hist_best", POINTER(c_double)),
                ("f_cap", c_int64), ("n_fhist", c_int64), ("ax_calls", c_int64),
                ("atr_calls", c_int64), ("syncs", c_int64), ("ax_sources", c_int64),
                ("stats", c_double * 8), ("record_waits", c_int64)]


class GlxAdmmOpts(ctypes.Structure):
    """glx_admm_opts (include/glx.h): the options of the dual ADMM solver."""
    _fields_ = [("maxit", c_int32), ("converge_len", c_int32), ("thres", c_double),
                ("tau", c_double), ("rho", c_double), ("fused", c_int32),
                ("max_total_iters", c_int64), ("reserved", c_int32 * 4)]


class GlxAdmmPrimalOpts(ctypes.Structure):
    """glx_admm_primal_opts (include/glx.h): the options of the primal ADMM solver."""
    _fields_ = [("maxit", c_int32), ("converge_len", c_int32), ("thres", c_double),
                ("tau", c_double), ("rho", c_double), ("eta_0", c_double), ("step_type", c_int32),
                ("form", c_int32), ("max_total_iters", c_int64), ("reserved", c_int32 * 4)]


class GlxAlmOpts(ctypes.Structure):
    """glx_alm_opts (include/glx.h): the options of the dual ALM solver."""
    _fields_ = [("maxit", c_int32), ("converge_len", c_int32), ("thres", c_double),
                ("tau", c_double), ("rho", c_double), ("inner_iters", c_int32),
                ("inner_step", c_double), ("fused", c_int32), ("max_total_iters", c_int64),
                ("reserved", c_int32 * 4)]


class GlxCertifiedInfo(ctypes.Structure):
    """glx_certified_info (include/glx.h): what glx_certified_solve reports."""
    _fields_ = [("iters", c_int64), ("checks", c_int64), ("compactions", c_int64), ("kept", c_int64),
                ("listed", c_int64), ("width", c_int64), ("rounds", c_int64), ("converged", c_int32), ("fused", c_int32),
                ("passes", c_double), ("tt", c_double), ("inner_rel_gap", c_double),
                ("cert", c_double * 8), ("kept_hist", c_int64 * 64)]


class GlxGroupCertifiedInfo(ctypes.Structure):
    """glx_group_certified_info (include/glx.h): what glx_group_certified_solve reports."""
    _fields_ = [("base", GlxCertifiedInfo), ("kept_groups", c_int64), ("listed_groups", c_int64),
                ("max_run", c_int64), ("reserved", c_int64)]


class GlxSglCertifiedInfo(ctypes.Structure):
    """glx_sgl_certified_info (include/glx.h): what glx_sgl_certified_solve reports."""
    _fields_ = [("base", GlxGroupCertifiedInfo), ("row_ratio", c_double), ("reserved", c_int64 * 3),
                ("kept_row_hist", c_int64 * 64)]


class GlxError(RuntimeError):
    """Error returned by libglx (message from glx_last_error())."""

    def __init__(self, code: int, msg: str):
        super().__init__("libglx error %d: %s" % (code, msg))
        self.code = code


_LIB = None

_SIGS = {
    "glx_abi_version": (c_int, []),
    "glx_last_error": (c_char_p, []),
    "glx_default_opts": (c_int, [c_int, POINTER(GlxOpts)]),
    "glx_workspace_bytes": (c_int, [POINTER(GlxProblem), POINTER(GlxOpts), POINTER(c_size_t)]),
    "glx_session_create": (c_int, [POINTER(c_void_p), POINTER(GlxProblem), POINTER(GlxOpts),
                                   c_void_p, c_size_t, c_void_p]),
    "glx_session_run": (c_int, [c_void_p, c_int64, POINTER(c_int64), POINTER(c_int32)]),
    "glx_session_finish": (c_int, [c_void_p, POINTER(GlxResult)]),
    "glx_session_kernel_time": (c_int, [c_void_p, c_int, POINTER(c_int64), POINTER(c_double)]),
    "glx_session_counters": (c_int, [c_void_p, POINTER(c_int64)]),
    "glx_session_ae_forms": (c_int, [c_void_p, POINTER(c_int64)]),
    "glx_session_progress": (c_int, [c_void_p, POINTER(c_int64)]),
    "glx_session_trace": (c_int, [c_void_p, POINTER(c_double), c_int64, POINTER(c_int64),
                                  POINTER(c_int64)]),
    "glx_session_describe": (c_int, [c_void_p, c_char_p, c_size_t]),
    "glx_mode_describe": (c_int, [POINTER(GlxProblem), POINTER(GlxOpts), c_char_p, c_size_t]),
    "glx_session_split_trace": (c_int, [c_void_p, POINTER(c_double), c_int64, POINTER(c_int64)]),
    "glx_session_destroy": (None, [c_void_p]),
    "glx_solve": (c_int, [POINTER(GlxProblem), POINTER(GlxOpts), c_void_p, c_size_t,
                          POINTER(GlxResult), c_void_p]),
    "glx_residual": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "glx_residual_batch": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_int,
                                   POINTER(c_void_p), c_void_p, POINTER(c_void_p), c_void_p,
                                   c_void_p, c_size_t, c_int, c_void_p]),
    "glx_gradient": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_size_t, c_void_p]),
    "glx_residual_gradient": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_int, POINTER(c_int), c_void_p]),
    "glx_residual_gradient2": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_size_t, c_int, POINTER(c_int), c_void_p]),
    "glx_prox": (c_int, [c_int, c_int64, c_int64, c_void_p, c_double, c_double, c_double,
                         c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_flagged_rows_product": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "glx_fused_ae_pass": (c_int, [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, POINTER(c_int), POINTER(c_int), c_void_p]),
    "glx_dense_pass_keep": (c_int, [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_int, POINTER(c_int), POINTER(c_int), c_void_p]),
    "glx_trial_mask_bytes": (c_int, [c_int64, POINTER(c_size_t)]),
    "glx_trial_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "glx_trial_proxgd": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_double, c_double, c_double, c_int, c_int, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                 c_void_p]),
    "glx_fin_atr_prox": (c_int, [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                 POINTER(c_int), c_void_p, c_void_p, c_double, c_double, c_double, c_int,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                 c_size_t, c_void_p]),
    "glx_fin_head_fits": (c_int, [c_int64, c_int, c_int]),
    "glx_session_fin_form": (c_int, [c_void_p, c_char_p, c_size_t]),
    "glx_trial_fista": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_double, c_double, c_double, c_double,
                                c_double, c_double, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_descent_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "glx_descent_step": (c_int, [c_int, c_int64, c_int64, c_int, c_void_p, c_int, c_double,
                                 c_double, c_double, c_double, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_size_t, c_void_p]),
    "glx_fgd_gradient": (c_int, [c_int, c_int64, c_int64, c_void_p, c_void_p, c_int, c_double,
                                 c_double, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_row_stats": (c_int, [c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t,
                              c_void_p]),
    "glx_threshold": (c_int, [c_int, c_int64, c_void_p, c_void_p, c_double, c_void_p, c_int,
                              c_void_p]),
    "glx_thr_combine": (c_int, [c_int, c_int64, c_void_p, c_void_p, c_void_p, c_double, c_double,
                                c_double, c_void_p]),
    "glx_descent_pass": (c_int, [c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_int,
                                 POINTER(c_int), c_void_p, c_size_t, c_void_p]),
    "glx_kernel_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "glx_plan_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_char_p, c_size_t]),
    "glx_admm_default_opts": (c_int, [POINTER(GlxAdmmOpts)]),
    "glx_admm_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(GlxAdmmOpts),
                                         POINTER(c_size_t)]),
    "glx_admm_dual_solve": (c_int, [POINTER(GlxProblem), c_void_p, POINTER(GlxAdmmOpts), c_void_p,
                                    c_size_t, POINTER(GlxResult), c_void_p]),
    "glx_admm_trace": (c_int, [POINTER(c_double), c_int64, POINTER(c_int64)]),
    "glx_admm_describe": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(GlxAdmmOpts), c_char_p,
                                  c_size_t]),
    "glx_admm_dual_step": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_double, c_double, c_double, c_int, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_gram": (c_int, [c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_sym_lambda_max": (c_int, [POINTER(c_double), c_int, POINTER(c_double)]),
    "glx_admm_primal_default_opts": (c_int, [POINTER(GlxAdmmPrimalOpts)]),
    "glx_admm_primal_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64,
                                                POINTER(GlxAdmmPrimalOpts), POINTER(c_size_t)]),
    "glx_admm_primal_describe": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(GlxAdmmPrimalOpts),
                                         c_char_p, c_size_t]),
    "glx_admm_primal_solve": (c_int, [POINTER(GlxProblem), c_void_p, c_void_p, c_void_p,
                                      POINTER(GlxAdmmPrimalOpts), c_void_p, c_size_t,
                                      POINTER(GlxResult), c_void_p]),
    "glx_admm_primal_step": (c_int, [c_int, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_double, c_double, c_double,
                                     c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_alm_default_opts": (c_int, [POINTER(GlxAlmOpts)]),
    "glx_alm_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(GlxAlmOpts),
                                        POINTER(c_size_t)]),
    "glx_alm_describe": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(GlxAlmOpts), c_char_p,
                                 c_size_t]),
    "glx_alm_dual_solve": (c_int, [POINTER(GlxProblem), c_void_p, c_void_p, POINTER(GlxAlmOpts), c_void_p,
                                   c_size_t, POINTER(GlxResult), c_void_p]),
    "glx_alm_inner_workspace_bytes": (c_int, [c_int, c_int64, c_int64, POINTER(c_size_t)]),
    "glx_alm_inner_step": (c_int, [c_int, c_int64, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                   c_void_p, c_double, c_double, c_double, c_double, c_int, c_void_p,
                                   c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_alm_inner_run": (c_int, [c_int, c_int64, c_int64, c_void_p, c_void_p, c_int, c_double, c_double,
                                  c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_admm_rhs": (c_int, [c_int, c_int64, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p]),
    "glx_admm_fin": (c_int, [c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_admm_primal_rhs": (c_int, [c_int, c_int64, c_void_p, c_void_p, c_void_p, c_double, c_void_p,
                                    c_void_p]),
    "glx_admm_primal_fin": (c_int, [c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_double, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_alm_j": (c_int, [c_int, c_int64, c_int, c_void_p, c_void_p, c_double, c_void_p, c_void_p]),
    "glx_alm_x": (c_int, [c_int, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_double, c_void_p,
                          c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_certificate_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "glx_certificate_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int, c_char_p, c_size_t]),
    "glx_certificate": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_double,
                                c_int, c_void_p, c_void_p, POINTER(c_double), c_void_p, c_size_t, c_void_p]),
    "glx_certificate_step": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_double, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),
    "glx_screen_guard": (c_int, [POINTER(c_double), c_double, c_int, c_int64, c_int64, c_int64, c_double,
                                 c_double, c_double, POINTER(c_double)]),
    "glx_screen_workspace_bytes": (c_int, [c_int64, c_int64, POINTER(c_size_t)]),
    "glx_col_norms": (c_int, [c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                              c_void_p]),
    "glx_screen_step": (c_int, [c_int64, c_void_p, c_void_p, c_double, c_double, c_double, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_gather_cols": (c_int, [c_int, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "glx_certified_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int, POINTER(c_size_t)]),
    "glx_certified_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int, c_char_p, c_size_t]),
    "glx_certified_solve": (c_int, [POINTER(GlxProblem), c_double, c_double, c_int64, c_int, c_int,
                                    c_void_p, POINTER(c_double), c_void_p, c_void_p, c_size_t,
                                    POINTER(GlxCertifiedInfo), c_void_p]),
    "glx_group_certificate_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64,
                                                      POINTER(c_size_t)]),
    "glx_group_certificate_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_char_p, c_size_t]),
    "glx_group_certificate": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_double,
                                      c_int64, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_double),
                                      c_void_p, c_size_t, c_void_p]),
    "glx_group_certified_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_int,
                                                    POINTER(c_size_t)]),
    "glx_group_certified_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_char_p,
                                             c_size_t]),
    "glx_group_certified_solve": (c_int, [POINTER(GlxProblem), c_int64, c_void_p, c_void_p, c_double, c_double,
                                          c_int64, c_int, c_int, c_void_p, POINTER(c_double), c_void_p,
                                          c_void_p, c_void_p, c_size_t, POINTER(GlxGroupCertifiedInfo),
                                          c_void_p]),
    "glx_group_screen_guard": (c_int, [POINTER(c_double), c_double, c_int, c_int64, c_int64, c_int64, c_int64,
                                       c_double, c_double, c_double, c_double, POINTER(c_double)]),
    "glx_group_workspace_bytes": (c_int, [c_int64, POINTER(c_size_t)]),
    "glx_group_step": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_int, c_void_p, c_double, c_double, c_double, c_double, c_double,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_group_certificate_step": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_size_t, c_void_p]),
    "glx_group_cnorm": (c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_size_t, c_void_p]),
    "glx_group_expand": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "glx_certificate_sw_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "glx_certificate_sw_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int, c_char_p, c_size_t]),
    "glx_certificate_sw": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_double,
                                   c_int, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_double),
                                   POINTER(c_double), c_void_p, c_size_t, c_void_p]),
    "glx_group_certificate_sw_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64,
                                                         POINTER(c_size_t)]),
    "glx_group_certificate_sw_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_char_p,
                                                  c_size_t]),
    "glx_group_certificate_sw": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                         c_double, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, POINTER(c_double), POINTER(c_double), c_void_p, c_size_t,
                                         c_void_p]),
    "glx_certified_sw_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int, POINTER(c_size_t)]),
    "glx_certified_sw_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int, c_char_p, c_size_t]),
    "glx_certified_solve_sw": (c_int, [POINTER(GlxProblem), c_void_p, c_void_p, c_double, c_double, c_int64,
                                       c_int, c_int, c_void_p, POINTER(c_double), c_void_p, c_void_p, c_size_t,
                                       POINTER(GlxCertifiedInfo), POINTER(c_double), c_void_p]),
    "glx_group_certified_sw_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_int,
                                                       POINTER(c_size_t)]),
    "glx_group_certified_sw_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_char_p,
                                                c_size_t]),
    "glx_group_certified_solve_sw": (c_int, [POINTER(GlxProblem), c_int64, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_double, c_double, c_int64, c_int, c_int, c_void_p,
                                             POINTER(c_double), c_void_p, c_void_p, c_void_p, c_size_t,
                                             POINTER(GlxGroupCertifiedInfo), POINTER(c_double), c_void_p]),
    "glx_screen_guard_sw": (c_int, [POINTER(c_double), c_double, c_int, c_int64, c_int64, c_int64, c_double,
                                    c_double, c_double, POINTER(c_double)]),
    "glx_group_screen_guard_sw": (c_int, [POINTER(c_double), c_double, c_int, c_int64, c_int64, c_int64,
                                          c_int64, c_double, c_double, c_double, c_double, POINTER(c_double)]),
    "glx_col_norms_sw": (c_int, [c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_size_t, c_void_p]),
    "glx_cert_fin_sw": (c_int, [c_int, c_int64, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_certificate_ic_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "glx_certificate_ic_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int, c_char_p, c_size_t]),
    "glx_certificate_ic": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_double,
                                   c_int, c_void_p, c_void_p, c_double, c_void_p, c_void_p, POINTER(c_double),
                                   POINTER(c_double), POINTER(c_double), c_void_p, c_size_t, c_void_p]),
    "glx_group_certificate_ic_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64,
                                                         POINTER(c_size_t)]),
    "glx_group_certificate_ic_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_char_p,
                                                  c_size_t]),
    "glx_group_certificate_ic": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                         c_double, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_double,
                                         c_void_p, c_void_p, POINTER(c_double), POINTER(c_double),
                                         POINTER(c_double), c_void_p, c_size_t, c_void_p]),
    "glx_certified_ic_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int, POINTER(c_size_t)]),
    "glx_certified_ic_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int, c_char_p, c_size_t]),
    "glx_certified_solve_ic": (c_int, [POINTER(GlxProblem), c_void_p, c_void_p, c_double, c_double, c_double,
                                       c_int64, c_int, c_int, c_void_p, POINTER(c_double), c_void_p, c_void_p,
                                       c_size_t, POINTER(GlxCertifiedInfo), POINTER(c_double), POINTER(c_double),
                                       c_void_p]),
    "glx_group_certified_ic_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_int,
                                                       POINTER(c_size_t)]),
    "glx_group_certified_ic_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_char_p,
                                                c_size_t]),
    "glx_group_certified_solve_ic": (c_int, [POINTER(GlxProblem), c_int64, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_double, c_double, c_double, c_int64, c_int, c_int,
                                             c_void_p, POINTER(c_double), c_void_p, c_void_p, c_void_p, c_size_t,
                                             POINTER(GlxGroupCertifiedInfo), POINTER(c_double),
                                             POINTER(c_double), c_void_p]),
    "glx_screen_guard_ic": (c_int, [POINTER(c_double), c_double, c_int, c_int64, c_int64, c_int64,
                                    POINTER(c_double), c_double, c_double, c_double, POINTER(c_double)]),
    "glx_group_screen_guard_ic": (c_int, [POINTER(c_double), c_double, c_int, c_int64, c_int64, c_int64,
                                          c_int64, c_double, c_double, POINTER(c_double), c_double, c_double,
                                          c_double, POINTER(c_double)]),
    "glx_intercept_workspace_bytes": (c_int, [c_int64, c_int64, POINTER(c_size_t)]),
    "glx_col_norms_ic": (c_int, [c_int, c_int64, c_int64, c_void_p, c_void_p, c_double, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_cert_fin_ic": (c_int, [c_int, c_int64, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_double,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_sgl_certificate_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, POINTER(c_size_t)]),
    "glx_sgl_certificate_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int, c_char_p, c_size_t]),
    "glx_sgl_certificate": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_double,
                                    c_double, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_double),
                                    c_void_p, c_size_t, c_void_p]),
    "glx_sgl_certificate_sw": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_double,
                                       c_double, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, POINTER(c_double), POINTER(c_double), c_void_p, c_size_t,
                                       c_void_p]),
    "glx_sgl_certified_workspace_bytes": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_int,
                                                  POINTER(c_size_t)]),
    "glx_sgl_certified_describe": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_char_p,
                                           c_size_t]),
    "glx_sgl_certified_solve": (c_int, [POINTER(GlxProblem), c_double, c_int64, c_void_p, c_void_p, c_double,
                                        c_double, c_int64, c_int, c_int, c_void_p, POINTER(c_double), c_void_p,
                                        c_void_p, c_void_p, c_size_t, POINTER(GlxSglCertifiedInfo), c_void_p]),
    "glx_sgl_certified_solve_sw": (c_int, [POINTER(GlxProblem), c_double, c_int64, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_double, c_double, c_int64, c_int, c_int, c_void_p,
                                           POINTER(c_double), c_void_p, c_void_p, c_void_p, c_size_t,
                                           POINTER(GlxSglCertifiedInfo), POINTER(c_double), c_void_p]),
    "glx_sgl_screen_guard": (c_int, [POINTER(c_double), c_double, c_double, c_double, c_int, c_int64, c_int64,
                                     c_int64, c_int64, c_double, c_double, c_double, c_double, POINTER(c_double)]),
    "glx_sgl_screen_guard_sw": (c_int, [POINTER(c_double), c_double, c_double, c_double, c_int, c_int64, c_int64,
                                        c_int64, c_int64, c_double, c_double, c_double, c_double,
                                        POINTER(c_double)]),
    "glx_sgl_step": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_int, c_void_p, c_double, c_double, c_double, c_double, c_double, c_double, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_sgl_certificate_step": (c_int, [c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_int, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_size_t, c_void_p]),
    "glx_sgl_dual_scale": (c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_double, c_double, c_double,
                                   c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_sgl_screen": (c_int, [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double,
                               c_double, c_double, c_double, c_double, c_double, c_int, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_size_t, c_void_p]),
    "glx_sgl_expand": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "glx_comm_unique_id": (c_int, [POINTER(c_uint8)]),
    "glx_comm_create": (c_int, [POINTER(c_void_p), POINTER(c_uint8), c_int, c_int]),
    "glx_comm_create_host": (c_int, [POINTER(c_void_p), c_int, c_int, c_void_p, c_void_p]),
    "glx_comm_allreduce": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "glx_comm_reduce_scatter": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "glx_comm_all_gather": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "glx_comm_progress": (c_int, [c_void_p, POINTER(c_int64)]),
    "glx_comm_destroy": (None, [c_void_p]),
}

EXPORTED = tuple(_SIGS)

# glx_host_allreduce_fn: int (*)(void* host_buf, int64_t count, int dtype, void* user)
HOST_ALLREDUCE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_int64, c_int, c_void_p)


def lib():
    """Load (once) and return the libglx handle; raise if it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libglx.so not found at %s — build it with "
                               "`python -c 'import __graft_entry__ as g; g.build()'` "
                               "(no CPU fallback exists)" % LIB_PATH)
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        if h.glx_abi_version() != 2:
            raise RuntimeError("libglx ABI mismatch")
        _LIB = h
    return _LIB


def check(rc: int):
    if rc != 0:
        msg = lib().glx_last_error()
        raise GlxError(rc, msg.decode() if msg else "?")
    return rc


def plan_describe(dtype: int, m: int, n: int, l: int) -> str:
    """The kernels and K splits libglx plans for this shape (see glx_plan_describe)."""
    buf = ctypes.create_string_buffer(512)
    check(lib().glx_plan_describe(dtype, m, n, l, buf, len(buf)))
    return buf.value.decode()


def mode_describe(problem: GlxProblem, opts: GlxOpts) -> str:
    """What a session of this problem and these options would describe (glx_mode_describe: resolved
    on the host, no device)."""
    buf = ctypes.create_string_buffer(1024)
    check(lib().glx_mode_describe(ctypes.byref(problem), ctypes.byref(opts), buf, len(buf)))
    return buf.value.decode()


def default_opts(method: int) -> GlxOpts:
    o = GlxOpts()
    check(lib().glx_default_opts(method, ctypes.byref(o)))
    return o


def admm_default_opts() -> GlxAdmmOpts:
    o = GlxAdmmOpts()
    check(lib().glx_admm_default_opts(ctypes.byref(o)))
    return o


def admm_describe(dtype: int, m: int, n: int, l: int, opts: "GlxAdmmOpts | None" = None) -> str:
    """The tiles of the dual ADMM solver's three passes and whether its row step is fused
    (glx_admm_describe: resolved on the host, no device)."""
    buf = ctypes.create_string_buffer(2048)
    check(lib().glx_admm_describe(dtype, m, n, l, ctypes.byref(opts) if opts is not None else None,
                                  buf, len(buf)))
    return buf.value.decode()


def alm_default_opts() -> GlxAlmOpts:
    o = GlxAlmOpts()
    check(lib().glx_alm_default_opts(ctypes.byref(o)))
    return o


def alm_describe(dtype: int, m: int, n: int, l: int, opts: "GlxAlmOpts | None" = None) -> str:
    """The tiles of the dual ALM solver's passes over K, A and Qn and whether its inner step is fused
    (glx_alm_describe: resolved on the host, no device). GlxError for what the solve refuses, fp32
    included."""
    buf = ctypes.create_string_buffer(2048)
    check(lib().glx_alm_describe(dtype, m, n, l, ctypes.byref(opts) if opts is not None else None,
                                 buf, len(buf)))
    return buf.value.decode()


def certificate_describe(dtype: int, m: int, n: int, l: int, fused: int = 0) -> str:
    """The tiles of the certificate's two passes and where its row terms run, "fused ..." or "row
    kernel ..." (glx_certificate_describe: resolved on the host, no device)."""
    buf = ctypes.create_string_buffer(2048)
    check(lib().glx_certificate_describe(dtype, m, n, l, int(fused), buf, len(buf)))
    return buf.value.decode()


def certified_describe(dtype: int, m: int, n: int, l: int, screen: bool = True) -> str:
    """The tiles of the certified solve's two passes at the full width, where its step runs and
    whether screening is on (glx_certified_describe: resolved on the host, no device)."""
    buf = ctypes.create_string_buffer(2048)
    check(lib().glx_certified_describe(dtype, m, n, l, int(bool(screen)), buf, len(buf)))
    return buf.value.decode()


def group_certificate_describe(dtype: int, m: int, n: int, l: int, max_run: int) -> str:
    """The tiles of the group certificate's two passes and the lane layout of its group kernel for
    runs of up to ``max_run`` rows (glx_group_certificate_describe: host only)."""
    buf = ctypes.create_string_buffer(2048)
    check(lib().glx_group_certificate_describe(dtype, m, n, l, int(max_run), buf, len(buf)))
    return buf.value.decode()


def group_certified_describe(dtype: int, m: int, n: int, l: int, max_run: int, screen: bool = True) -> str:
    """:func:`certified_describe` for the grouped solve (glx_group_certified_describe: host only)."""
    buf = ctypes.create_string_buffer(2048)
    check(lib().glx_group_certified_describe(dtype, m, n, l, int(max_run), int(bool(screen)), buf, len(buf)))
    return buf.value.decode()


def admm_primal_default_opts() -> GlxAdmmPrimalOpts:
    o = GlxAdmmPrimalOpts()
    check(lib().glx_admm_primal_default_opts(ctypes.byref(o)))
    return o


def admm_primal_describe(dtype: int, m: int, n: int, l: int,
                         opts: "GlxAdmmPrimalOpts | None" = None) -> str:
    """The resolved form ("form=direct" or "form=Woodbury") and the tiles of the primal ADMM solver's
    passes (glx_admm_primal_describe: resolved on the host, no device). GlxError for what the solve
    refuses, the fp32 rule included."""
    buf = ctypes.create_string_buffer(2048)
    check(lib().glx_admm_primal_describe(dtype, m, n, l, ctypes.byref(opts) if opts is not None else None,
                                         buf, len(buf)))
    return buf.value.decode()
