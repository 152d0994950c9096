"""Host side of the primal ADMM solver: ``gl_Admm_primal(x0, A, b, mu, opts) -> (x, k, out)``.

Mirrors the reference's ``code/gl_ADMM_primal.py:10-117``:

* ``opts`` is merged over the defaults exactly like ``{**default_opts, **opts}`` (``:23``): unknown
  keys are ignored (``converge_thres``, which the reference reads and never uses, among them), the
  caller's dict is not mutated.
* ``x0`` is copied (``:53``); ``A`` and ``b`` are read-only.
* returns ``(x, k, out)`` with ``out = {"tt", "fval", "f_hist", "f_hist_best"}`` (``:110-115``) plus
  ``out["glx"]``; ``x`` comes back as the caller's array type.

The reference factors ``rho I + A^T A`` (n x n) once (``:62``) and solves with the triangular
factors at every iteration (``:78``). Here the setup forms an explicit inverse once, always in
float64, with torch on the device (plumbing, like :func:`glx.admm.inverse_factor`), casts it to A's
dtype and hands it to libglx (``csrc/admm_primal.cpp``), in one of two forms:

* direct (``form=1``): ``Kn = (rho I + A^T A)^-1`` (n x n);
* Woodbury (``form=2``): ``K = (rho I + A A^T)^-1`` (m x m), with
  ``(rho I + A^T A)^-1 w = (w - A^T K (A w)) / rho``.

``form=0`` (the default) takes Woodbury exactly when ``m^2 + m n < n^2``. float32 is admitted only
for m >= n in the direct form (the conditioning of ``rho I + A^T A`` for m < n is beyond float32:
the solver would never meet its stop rule); anything else raises before the setup is spent.
``out["tt"]`` includes the setup, as the reference's stopwatch starts before its Cholesky;
``out["glx"]["setup_s"]`` reports it separately. There is no CPU path.

Build-only option keys (ignored by the reference): ``form``, ``max_total_iters``, ``device``.
"""
from __future__ import annotations

import ctypes
import logging
import time
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import GlxAdmmPrimalOpts, GlxProblem, GlxResult, check, lib
from .admm import _trace
from .solver import _as_device, _device, _dtype_of

logger = logging.getLogger("opt")

_REF_KEYS = ("maxit", "thres", "tau", "rho", "eta_0", "converge_len")
_BUILD_KEYS = ("form", "max_total_iters")
_STEP_TYPES = {"fixed": 1, "diminishing": 2, "diminishing2": 3}
FORMS = {1: "direct", 2: "Woodbury"}


def make_opts(opts: Dict[str, Any]) -> GlxAdmmPrimalOpts:
    """The reference's default_opts (gl_ADMM_primal.py:11-20) overridden by ``opts``."""
    o = _lib.admm_primal_default_opts()
    for key in _REF_KEYS + _BUILD_KEYS:
        if key in opts:
            setattr(o, key, type(getattr(o, key))(opts[key]))
    if "step_type" in opts:
        st = opts["step_type"]
        if st not in _STEP_TYPES:
            raise ValueError("step_type must be one of %s, got %r" % (sorted(_STEP_TYPES), st))
        o.step_type = _STEP_TYPES[st]
    return o


def resolved_form(dtype: int, m: int, n: int, l: int, o: Optional[GlxAdmmPrimalOpts] = None) -> int:
    """1 (direct) or 2 (Woodbury), as libglx resolves it; GlxError for what the solve refuses."""
    return 2 if _lib.admm_primal_describe(dtype, m, n, l, o).startswith("form=Woodbury") else 1


def setup(A: torch.Tensor, b: torch.Tensor, rho: float, form: int):
    """(K, ATb, AATb) for the resolved ``form`` through a float64 Cholesky factor, cast to A's dtype:
    direct: K = (rho I + A^T A)^-1 (n x n), AATb None; Woodbury: K = (rho I + A A^T)^-1 (m x m)."""
    a = A if A.dtype == torch.float64 else A.to(torch.float64)
    bb = b if b.dtype == torch.float64 else b.to(torch.float64)
    ATb = a.T @ bb
    if form == 2:
        M = a @ a.T
        AATb = (a @ ATb).to(A.dtype).contiguous()
    else:
        M = a.T @ a
        AATb = None
    M.diagonal().add_(float(rho))
    K = torch.cholesky_inverse(torch.linalg.cholesky(M))
    return K.to(A.dtype).contiguous(), ATb.to(A.dtype).contiguous(), AATb


def workspace(dtype: int, m: int, n: int, l: int, o: Optional[GlxAdmmPrimalOpts], device) -> torch.Tensor:
    nbytes = ctypes.c_size_t(0)
    check(lib().glx_admm_primal_workspace_bytes(dtype, m, n, l, ctypes.byref(o) if o is not None else None,
                                                ctypes.byref(nbytes)))
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def solve(x0, A, b, mu, opts: Optional[Dict[str, Any]] = None) -> Tuple[Any, int, Dict[str, Any]]:
    """Run the primal ADMM solver on the GPU; reference-compatible return."""
    opts = dict(opts or {})
    lib()  # fail loudly before touching data if the library is missing
    o = make_opts(opts)
    dtype = _dtype_of(A)
    gdt = _lib.GLX_F64 if dtype == torch.float64 else _lib.GLX_F32
    shape_a, shape_b, shape_x = tuple(np.shape(A)), tuple(np.shape(b)), tuple(np.shape(x0))
    if len(shape_a) != 2 or len(shape_b) != 2 or len(shape_x) != 2:
        raise ValueError("A, b and x0 must be 2-D (group lasso with l columns)")
    m, n = shape_a
    l = shape_x[1]
    if shape_b != (m, l) or shape_x[0] != n:
        raise ValueError("shape mismatch: A %s, b %s, x0 %s" % (shape_a, shape_b, shape_x))
    plan = _lib.admm_primal_describe(gdt, m, n, l, o)   # raises what the solve refuses, before the setup
    form = 2 if plan.startswith("form=Woodbury") else 1
    device = _device(opts)
    numpy_in = not isinstance(x0, torch.Tensor)
    Ad = _as_device(A, device, dtype)
    bd = _as_device(b, device, dtype)
    xd = _as_device(x0, device, dtype).clone()      # x_k = np.copy(x0)  (gl_ADMM_primal.py:53)
    stream = torch.cuda.current_stream(device)
    with torch.cuda.device(device):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        K, ATb, AATb = setup(Ad, bd, o.rho, form)
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
        check(lib().glx_admm_primal_solve(ctypes.byref(p), ctypes.c_void_p(K.data_ptr()),
                                          ctypes.c_void_p(ATb.data_ptr()),
                                          ctypes.c_void_p(AATb.data_ptr()) if AATb is not None else None,
                                          ctypes.byref(o), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                          ctypes.byref(res), ctypes.c_void_p(stream.cuda_stream)))
        torch.cuda.synchronize(device)
    nh = int(res.n_fhist)
    f_hist = [np.float64(v) for v in fh[:nh]]
    if logger.isEnabledFor(logging.DEBUG):   # gl_ADMM_primal.py:96-97, replayed after the solve
        for it, (f, s) in enumerate(zip(f_hist, _trace()), start=1):
            logger.debug("iter= {:5}, objective= {:10E}, sparsity= {:3f}".format(it, float(f), float(s)))
    x = xd.cpu().numpy() if numpy_in else xd
    out = {"tt": float(res.tt) + setup_s, "fval": np.float64(res.fval), "f_hist": f_hist,
           "f_hist_best": [np.float64(v) for v in fb[:nh]],
           "glx": {"setup_s": setup_s, "loop_s": float(res.tt), "form": FORMS[int(res.stats[1])],
                   "k_calls": int(res.stats[0]), "ax_calls": int(res.ax_calls),
                   "atr_calls": int(res.atr_calls), "syncs": int(res.syncs), "plan": plan}}
    return x, int(res.iters), out
