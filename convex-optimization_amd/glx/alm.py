"""Host side of the dual ALM solver: ``gl_Alm_dual(x0, A, b, mu, opts) -> (x, k, out)``.

Mirrors the reference's ``code/gl_ALM_dual.py:66-158``:

* ``opts`` is merged over the defaults exactly like ``{**default_opts, **opts}`` (``:76``): unknown
  keys are ignored, the caller's dict is not mutated.
* ``x0`` is copied (``:104``); ``A`` and ``b`` are read-only.
* returns ``(x, k, out)`` with ``out = {"tt", "fval", "f_hist", "f_hist_best"}`` (``:151-156``) plus
  ``out["glx"]``; ``x`` comes back as the caller's array type.

The reference rebuilds an m x m inverse, the n x n matrix Q and J at every outer iteration
(``:33-40``). Here the setup forms, once per solve, always in float64, with torch on the device
(plumbing, like ``alpha0 = 1 / lambda_max`` in :mod:`glx.solver`):

* ``K = (I + rho A A^T)^-1`` (:func:`glx.admm.inverse_factor`), and
* ``Qn = rho (I + rho A^T A)^-1 = rho (I - A^T (rho K A))`` from K by the Woodbury identity,
  symmetrised: no second factorisation, and the form the deviation from the reference was measured
  with ("Dual ALM").

libglx's native loop (``csrc/alm.cpp``) then runs the outer iteration with the 500-step inner loop
enqueued on the device. ``out["tt"]`` includes the setup, as the reference's stopwatch starts before
its Cholesky; ``out["glx"]["setup_s"]`` reports it separately. float64 only: float32 input is
refused (GLX_E_INVALID). There is no CPU path.

Build-only option keys (ignored by the reference): ``inner_iters`` (500) and ``inner_step`` (1e-2),
the reference's hard-coded ``max_iteration`` and ``t``; ``fused`` (0 auto, 1 on, 2 off: the inner
step in the epilogue of Qn y); ``max_total_iters``; ``device``. As in the reference nothing guards
``inner_step * rho > 1``.
"""
from __future__ import annotations

import ctypes
import logging
import time
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import GlxAlmOpts, GlxProblem, GlxResult, check, lib
from .admm import _trace, inverse_factor
from .solver import _as_device, _device, _dtype_of

logger = logging.getLogger("opt")

_REF_KEYS = ("maxit", "thres", "tau", "rho", "converge_len")
_BUILD_KEYS = ("inner_iters", "inner_step", "fused", "max_total_iters")


def make_opts(opts: Dict[str, Any]) -> GlxAlmOpts:
    """The reference's default_opts (gl_ALM_dual.py:67-73) overridden by ``opts``."""
    o = _lib.alm_default_opts()
    for key in _REF_KEYS + _BUILD_KEYS:
        if key in opts:
            setattr(o, key, type(getattr(o, key))(opts[key]))
    return o


def inner_matrix(A: torch.Tensor, K: torch.Tensor, rho: float) -> torch.Tensor:
    """Qn = rho (I + rho A^T A)^-1 (n x n, float64, symmetric) from K = (I + rho A A^T)^-1 by
    Woodbury: rho (I - A^T (rho K A))."""
    a = A.to(torch.float64)
    n = a.shape[1]
    F = float(rho) * (K.to(torch.float64) @ a)
    Q = float(rho) * (torch.eye(n, dtype=torch.float64, device=a.device) - a.T @ F)
    return (0.5 * (Q + Q.T)).contiguous()


def workspace(dtype: int, m: int, n: int, l: int, o: Optional[GlxAlmOpts], device) -> torch.Tensor:
    nbytes = ctypes.c_size_t(0)
    check(lib().glx_alm_workspace_bytes(dtype, m, n, l, ctypes.byref(o) if o is not None else None,
                                        ctypes.byref(nbytes)))
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def solve(x0, A, b, mu, opts: Optional[Dict[str, Any]] = None) -> Tuple[Any, int, Dict[str, Any]]:
    """Run the dual ALM solver on the GPU; reference-compatible return."""
    opts = dict(opts or {})
    lib()  # fail loudly before touching data if the library is missing
    dtype = _dtype_of(A)
    numpy_in = not isinstance(x0, torch.Tensor)
    gdt = _lib.GLX_F64 if dtype == torch.float64 else _lib.GLX_F32
    o = make_opts(opts)
    if np.ndim(x0) != 2 or np.ndim(A) != 2 or np.ndim(b) != 2:
        raise ValueError("A, b and x0 must be 2-D (group lasso with l columns)")
    m, n = A.shape
    l = x0.shape[1]
    if tuple(b.shape) != (m, l) or x0.shape[0] != n:
        raise ValueError("shape mismatch: A %s, b %s, x0 %s" % (tuple(A.shape), tuple(b.shape),
                                                                 tuple(x0.shape)))
    _lib.alm_describe(gdt, m, n, l, o)   # refuses fp32 (and l > 32) before a device is touched
    device = _device(opts)
    Ad = _as_device(A, device, dtype)
    bd = _as_device(b, device, dtype)
    xd = _as_device(x0, device, dtype).clone()      # x_k = np.copy(x0)  (gl_ALM_dual.py:104)
    stream = torch.cuda.current_stream(device)
    with torch.cuda.device(device):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        K = inverse_factor(Ad, o.rho)
        Qn = inner_matrix(Ad, K, o.rho)
        torch.cuda.synchronize(device)
        setup_s = time.perf_counter() - t0
        ws = workspace(gdt, m, n, l, o, device)
        p = GlxProblem(dtype=gdt, method=0, m=m, n=n, l=l, A=Ad.data_ptr(), b=bd.data_ptr(),
                       x=xd.data_ptr(), mu0=float(mu), comm=None)
        cap = max(1, int(o.maxit))
        fh = np.zeros(cap, dtype=np.float64)
        fb = np.zeros(cap, dtype=np.float64)
        res = GlxResult(f_hist=fh.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                        f_hist_best=fb.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), f_cap=cap)
        check(lib().glx_alm_dual_solve(ctypes.byref(p), ctypes.c_void_p(K.data_ptr()),
                                       ctypes.c_void_p(Qn.data_ptr()), ctypes.byref(o),
                                       ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.byref(res),
                                       ctypes.c_void_p(stream.cuda_stream)))
        torch.cuda.synchronize(device)
    nh = int(res.n_fhist)
    f_hist = [np.float64(v) for v in fh[:nh]]
    if logger.isEnabledFor(logging.DEBUG):   # gl_ALM_dual.py:137-138, replayed after the solve
        for it, (f, s) in enumerate(zip(f_hist, _trace()), start=1):
            logger.debug("iter= {:5}, objective= {:10E}, sparsity= {:3f}".format(it, float(f), float(s)))
    x = xd.cpu().numpy() if numpy_in else xd
    out = {"tt": float(res.tt) + setup_s, "fval": np.float64(res.fval), "f_hist": f_hist,
           "f_hist_best": [np.float64(v) for v in fb[:nh]],
           "glx": {"setup_s": setup_s, "loop_s": float(res.tt), "ax_calls": int(res.ax_calls),
                   "atr_calls": int(res.atr_calls), "k_calls": int(res.stats[0]),
                   "syncs": int(res.syncs), "fused": bool(res.stats[1]),
                   "inner_steps": int(res.stats[2]), "plan": _lib.alm_describe(gdt, m, n, l, o)}}
    return x, int(res.iters), out
