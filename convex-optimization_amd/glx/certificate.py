"""An optimality certificate for any iterate of the group-lasso problem, on the GPU.

For ``P(x) = 1/2 ||A x - b||_F^2 + mu sum_i ||x_i||_2`` (``x_i`` the rows of the n x l iterate) the
dual is ``D(theta) = -1/2 ||theta||_F^2 - <theta, b>`` over ``||(A^T theta)_i||_2 <= mu``. With
``r = A x - b``, ``g = A^T r``, ``gmax = max_i ||g_i||_2`` and ``s = 1`` where ``gmax <= mu``,
``mu / gmax`` elsewhere, ``theta = s r`` is dual feasible, so

    gap = P(x) - D(s r) = 1/2 (1 + s^2) ||r||^2 + s <r, b> + mu sum_i ||x_i||  >=  P(x) - min P  >=  0

is a rigorous bound on the suboptimality of ``x``. It costs one pass over A and one over A^T
(libglx's ``glx_certificate``, ``csrc/certificate.cpp``); the host composes the figures below in
float64 from the eight-value record the device returns. There is no CPU path.

The bound is valid for every x but can be loose: where gmax sits a little above a tiny mu the
rescaling ``s`` throws most of ``r`` away (0.2 to 0.96 of P at the ADMM solvers' recorded results,
against 2e-4 to 1e-3 of P for ALM's). That is why the KKT violation is reported beside it: for row i,
``||g_i + mu x_i / ||x_i|| ||`` where ``x_i != 0`` and ``max(||g_i|| - mu, 0)`` where ``x_i = 0``;
``kkt_max`` is the largest and ``kkt_fro`` the root of the sum of squares.
"""
from __future__ import annotations

import ctypes
import math
import sys
from typing import Any, Dict

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .solver import _as_device, _device, _dtype_of

_TINY = sys.float_info.min


def workspace(dtype: int, m: int, n: int, l: int, device) -> torch.Tensor:
    nbytes = ctypes.c_size_t(0)
    check(lib().glx_certificate_workspace_bytes(dtype, m, n, l, ctypes.byref(nbytes)))
    return torch.empty(int(nbytes.value), dtype=torch.uint8, device=device)


def compose(rec, mu: float) -> Dict[str, Any]:
    """The certificate's figures from the record [||r||^2, <r, b>, sum_i ||x_i||, gmax, kkt_max,
    sum_i kkt_i^2, nonzero rows, fused was used] and mu, in float64."""
    rr, rb, sx, gmax, kmax, ksq, nz, fused = (float(v) for v in rec)
    mu = float(mu)
    scale = 1.0 if gmax <= mu else mu / gmax      # (a NaN gmax gives a NaN scale)
    primal = 0.5 * rr + mu * sx
    dual = -0.5 * scale * scale * rr - scale * rb
    gap = primal - dual
    return {"primal": primal, "dual": dual, "gap": gap, "rel_gap": gap / max(abs(primal), _TINY),
            "scale": scale, "gmax": gmax, "kkt_max": kmax, "kkt_fro": math.sqrt(ksq),
            "nonzero_rows": nz if math.isnan(nz) else int(nz), "fused": bool(fused)}


def _record(xd: torch.Tensor, Ad: torch.Tensor, bd: torch.Tensor, mu: float, fused: int, row_norms: bool):
    m, n = Ad.shape
    l = xd.shape[1]
    device = Ad.device
    gdt = _lib.GLX_F64 if Ad.dtype == torch.float64 else _lib.GLX_F32
    rec = (ctypes.c_double * 8)()
    with torch.cuda.device(device):
        ws = workspace(gdt, m, n, l, device)
        rn = torch.empty(n, dtype=torch.float64, device=device) if row_norms else None
        check(lib().glx_certificate(gdt, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), float(mu),
                                    int(fused), None, None if rn is None else rn.data_ptr(), rec,
                                    ws.data_ptr(), ws.numel(),
                                    ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    return list(rec), rn, _lib.certificate_describe(gdt, m, n, l, fused)


def _inputs(x, A, b):
    lib()  # fail loudly before touching data if the library is missing
    device = A.device if isinstance(A, torch.Tensor) and A.is_cuda else _device({})
    dtype = _dtype_of(A)
    Ad = _as_device(A, device, dtype)
    bd = _as_device(b, device, dtype)
    if Ad.dim() != 2 or bd.dim() != 2:
        raise ValueError("A and b must be 2-D (group lasso with l columns)")
    m, n = Ad.shape
    l = bd.shape[1]
    if bd.shape[0] != m:
        raise ValueError("shape mismatch: A %s, b %s" % (tuple(Ad.shape), tuple(bd.shape)))
    if x is None:
        xd = torch.zeros((n, l), dtype=dtype, device=device)
    else:
        xd = _as_device(x, device, dtype)
        if xd.dim() != 2 or tuple(xd.shape) != (n, l):
            raise ValueError("shape mismatch: A %s, b %s, x %s" % (tuple(Ad.shape), tuple(bd.shape),
                                                                    tuple(xd.shape)))
    return xd, Ad, bd


def record(x, A, b, mu, *, fused: int = 0) -> np.ndarray:
    """The raw record of glx_certificate, eight float64 values: [||r||^2, <r, b>, sum_i ||x_i||, gmax,
    kkt_max, sum_i kkt_i^2, nonzero rows, fused was used] (what :func:`compose` reads)."""
    xd, Ad, bd = _inputs(x, A, b)
    return np.asarray(_record(xd, Ad, bd, float(mu), fused, False)[0], dtype=np.float64)


def certificate(x, A, b, mu, *, fused: int = 0, row_norms: bool = False) -> Dict[str, Any]:
    """The duality gap and KKT violation of the iterate ``x`` at ``mu`` (module docstring).

    ``x`` (n x l), ``A`` (m x n) and ``b`` (m x l) are NumPy arrays or torch tensors and are not
    modified; the computation runs in A's dtype. ``fused``: 0 auto, 1 the row terms in the epilogue of
    A^T r where the plan admits it, 2 a row kernel behind the plain product (the same bits). Returns
    ``primal``, ``dual``, ``gap`` (>= primal - min P up to rounding), ``rel_gap`` = gap /
    max(|primal|, tiny), ``scale`` (s), ``gmax``, ``kkt_max``, ``kkt_fro``, ``nonzero_rows``,
    ``fused`` (whether the fused form ran), ``plan`` (glx_certificate_describe's line) and, with
    ``row_norms=True``, ``row_norms``: ||g_i||_2 for every row, a float64 array of length n (NumPy
    for NumPy inputs, a device tensor otherwise)."""
    mu = float(mu)
    if not mu >= 0.0:
        raise ValueError("mu must be >= 0")
    xd, Ad, bd = _inputs(x, A, b)
    rec, rn, plan = _record(xd, Ad, bd, mu, fused, row_norms)
    out = compose(rec, mu)
    out["plan"] = plan
    if row_norms:
        out["row_norms"] = rn if isinstance(A, torch.Tensor) else rn.cpu().numpy()
    return out


def mu_max(A, b) -> float:
    """The smallest mu for which x = 0 is optimal, max_i ||(A^T b)_i||_2: the certificate's gmax at
    x = 0, where r = -b."""
    xd, Ad, bd = _inputs(None, A, b)
    rec, _, _ = _record(xd, Ad, bd, 0.0, 0, False)
    return float(rec[3])
