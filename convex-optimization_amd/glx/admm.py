"""Host side of the dual ADMM solver: ``gl_Admm_dual(x0, A, b, mu, opts) -> (x, k, out)``.

Mirrors the reference's ``code/gl_ADMM_dual.py:10-103``:

* ``opts`` is merged over the defaults exactly like ``{**default_opts, **opts}`` (``:20``): unknown
  keys are ignored, the caller's dict is not mutated.
* ``x0`` is copied (``:48``); ``A`` and ``b`` are read-only.
* returns ``(x, k, out)`` with ``out = {"tt", "fval", "f_hist", "f_hist_best"}`` (``:96-101``) plus
  ``out["glx"]``; ``x`` comes back as the caller's array type.

The reference factors ``I + rho A A^T`` once (``:57``) and solves with the triangular factors at
every iteration (``:63``). Here the setup forms the explicit inverse
``K = cholesky_inverse(cholesky(I + rho A A^T))`` once, always in float64, with torch on the
device (plumbing, like ``alpha0 = 1 / lambda_max`` in :mod:`glx.solver`), casts it to A's dtype
and hands it to libglx, whose native loop (``csrc/admm.cpp``) then runs one product with K and
two passes over A per iteration. ``out["tt"]`` includes the setup, as the reference's stopwatch
starts before its Cholesky; ``out["glx"]["setup_s"]`` reports it separately. There is no CPU path.

With A in float32 and m > n, K cast to float32 costs about 1e-3 of the objective (I + rho A A^T
is then ill-conditioned: A A^T is rank-deficient); use float64 there.

Build-only option keys (ignored by the reference): ``fused`` (0 auto, 1 on, 2 off: the row step in
the epilogue of A^T z), ``max_total_iters``, ``device``.
"""
from __future__ import annotations

import ctypes
import logging
import time
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import GlxAdmmOpts, GlxProblem, GlxResult, check, lib
from .solver import _as_device, _device, _dtype_of

logger = logging.getLogger("opt")

_REF_KEYS = ("maxit", "thres", "tau", "rho", "converge_len")
_BUILD_KEYS = ("fused", "max_total_iters")


def make_opts(opts: Dict[str, Any]) -> GlxAdmmOpts:
    """The reference's default_opts (gl_ADMM_dual.py:11-17) overridden by ``opts``."""
    o = _lib.admm_default_opts()
    for key in _REF_KEYS + _BUILD_KEYS:
        if key in opts:
            setattr(o, key, type(getattr(o, key))(opts[key]))
    return o


def inverse_factor(A: torch.Tensor, rho: float) -> torch.Tensor:
    """K = (I + rho A A^T)^-1 (m x m) through a float64 Cholesky factor, cast to A's dtype."""
    a = A if A.dtype == torch.float64 else A.to(torch.float64)
    m = a.shape[0]
    M = torch.eye(m, dtype=torch.float64, device=a.device) + float(rho) * (a @ a.T)
    K = torch.cholesky_inverse(torch.linalg.cholesky(M))
    return K.to(A.dtype).contiguous()


def workspace(dtype: int, m: int, n: int, l: int, o: Optional[GlxAdmmOpts], device) -> torch.Tensor:
    nbytes = ctypes.c_size_t(0)
    check(lib().glx_admm_workspace_bytes(dtype, m, n, l, ctypes.byref(o) if o is not None else None,
                                         ctypes.byref(nbytes)))
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def _trace() -> np.ndarray:
    n = ctypes.c_int64(0)
    check(lib().glx_admm_trace(None, 0, ctypes.byref(n)))
    sp = np.zeros(int(n.value), dtype=np.float64)
    if n.value:
        check(lib().glx_admm_trace(sp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(n.value),
                                   ctypes.byref(n)))
    return sp


def solve(x0, A, b, mu, opts: Optional[Dict[str, Any]] = None) -> Tuple[Any, int, Dict[str, Any]]:
    """Run the dual ADMM solver on the GPU; reference-compatible return."""
    opts = dict(opts or {})
    lib()  # fail loudly before touching data if the library is missing
    device = _device(opts)
    dtype = _dtype_of(A)
    numpy_in = not isinstance(x0, torch.Tensor)
    Ad = _as_device(A, device, dtype)
    bd = _as_device(b, device, dtype)
    xd = _as_device(x0, device, dtype).clone()      # x_k = np.copy(x0)  (gl_ADMM_dual.py:48)
    if Ad.dim() != 2 or bd.dim() != 2 or xd.dim() != 2:
        raise ValueError("A, b and x0 must be 2-D (group lasso with l columns)")
    m, n = Ad.shape
    l = xd.shape[1]
    if bd.shape != (m, l) or xd.shape[0] != n:
        raise ValueError("shape mismatch: A %s, b %s, x0 %s" % (tuple(Ad.shape), tuple(bd.shape),
                                                                 tuple(xd.shape)))
    o = make_opts(opts)
    gdt = _lib.GLX_F64 if dtype == torch.float64 else _lib.GLX_F32
    stream = torch.cuda.current_stream(device)
    with torch.cuda.device(device):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        K = inverse_factor(Ad, o.rho)
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
        check(lib().glx_admm_dual_solve(ctypes.byref(p), ctypes.c_void_p(K.data_ptr()), ctypes.byref(o),
                                        ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.byref(res),
                                        ctypes.c_void_p(stream.cuda_stream)))
        torch.cuda.synchronize(device)
    nh = int(res.n_fhist)
    f_hist = [np.float64(v) for v in fh[:nh]]
    if logger.isEnabledFor(logging.DEBUG):   # gl_ADMM_dual.py:82-83, replayed after the solve
        for it, (f, s) in enumerate(zip(f_hist, _trace()), start=1):
            logger.debug("iter= {:5}, objective= {:10E}, sparsity= {:3f}".format(it, float(f), float(s)))
    x = xd.cpu().numpy() if numpy_in else xd
    out = {"tt": float(res.tt) + setup_s, "fval": np.float64(res.fval), "f_hist": f_hist,
           "f_hist_best": [np.float64(v) for v in fb[:nh]],
           "glx": {"setup_s": setup_s, "loop_s": float(res.tt), "ax_calls": int(res.ax_calls),
                   "atr_calls": int(res.atr_calls), "k_calls": int(res.stats[0]),
                   "syncs": int(res.syncs), "fused": bool(res.stats[1]),
                   "plan": _lib.admm_describe(gdt, m, n, l, o)}}
    return x, int(res.iters), out
