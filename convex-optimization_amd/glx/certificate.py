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

Feature groups and weights (``groups=``, ``weights=``): the classical group lasso
``P(x) = 1/2 ||A x - b||_F^2 + mu sum_g w_g ||x_[g]||_F`` over contiguous row ranges of x, given as
a ``group_ptr`` array of G + 1 offsets (``group_ptr[0] = 0``, ``group_ptr[G] = n``, strictly
increasing) and G weights ``w_g > 0`` (default 1). ``weights`` alone makes every row its own group:
a weighted row lasso. Everything above carries over with "row" read as "group" and mu as mu w_g:
the constraint is ``||(A^T theta)_[g]|| <= mu w_g``, ``gmax = max_g ||g_[g]|| / w_g``, and
``nonzero_groups`` replaces ``nonzero_rows``. Labels that are not contiguous are the caller's to
sort: :func:`group_order` gives the permutation and the offsets, the caller passes ``A[:, perm]``
and un-permutes x; the library never gathers A for this.
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


def group_order(labels):
    """Contiguous groups from arbitrary labels, on the host: ``(perm, group_ptr)`` with ``perm`` the
    stable argsort of ``labels`` (rows of one label keep their order, labels ascend) and
    ``group_ptr`` (int32, G + 1) the offsets of the sorted labels' runs. Solve with ``A[:, perm]`` and
    ``groups=group_ptr``; then ``x[perm] = x_sorted`` puts the rows back."""
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.size == 0:
        raise ValueError("labels must be a non-empty 1-D array")
    perm = np.argsort(lab, kind="stable")
    srt = lab[perm]
    starts = np.flatnonzero(np.concatenate(([True], srt[1:] != srt[:-1])))
    return perm.astype(np.int64), np.concatenate((starts, [lab.size])).astype(np.int32)


def check_groups(groups, weights, n: int, l: int = 1):
    """The host-side checks of ``groups`` / ``weights`` for an n-row iterate, before any device work.
    Returns None where both are None (the row problem), else ``(group_ptr int32 (G + 1), weights
    float64 (G))`` with the defaults filled in: single rows for ``groups=None``, 1 for
    ``weights=None``. ValueError for offsets that do not start at 0, do not end at n or are not
    strictly increasing, for a weight that is <= 0, NaN or infinite, for a length mismatch and for
    l > 128."""
    if groups is None and weights is None:
        return None
    n = int(n)
    if int(l) > 128:
        raise ValueError("groups: l <= 128")
    if groups is None:
        ptr = np.arange(n + 1, dtype=np.int64)
    else:
        if isinstance(groups, torch.Tensor):
            groups = groups.cpu().numpy()
        ptr = np.asarray(groups)
        if ptr.ndim != 1 or ptr.size < 2:
            raise ValueError("groups must be a 1-D group_ptr array of G + 1 >= 2 offsets")
        if not np.issubdtype(ptr.dtype, np.integer):
            raise ValueError("groups must hold integers")
        ptr = ptr.astype(np.int64)
        if ptr[0] != 0:
            raise ValueError("groups: group_ptr[0] must be 0")
        if ptr[-1] != n:
            raise ValueError("groups: group_ptr[G] must be n = %d (is %d)" % (n, int(ptr[-1])))
        if np.any(np.diff(ptr) < 1):
            raise ValueError("groups: group_ptr must be strictly increasing")
    G = ptr.size - 1
    if weights is None:
        w = np.ones(G, dtype=np.float64)
    else:
        if isinstance(weights, torch.Tensor):
            weights = weights.cpu().numpy()
        w = np.asarray(weights, dtype=np.float64)
        if w.ndim != 1 or w.size != G:
            raise ValueError("weights must have one entry per group (%d), got shape %s" % (G, tuple(w.shape)))
        if not np.all(np.isfinite(w)) or np.any(w <= 0.0):
            raise ValueError("every weight must be positive and finite")
    return np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(w)


def check_row_ratio(row_ratio, gw, fit_intercept: bool = False) -> float:
    """The host-side check of ``row_ratio`` (the sparse-group penalty's tau), before any device work.
    None and 0 come back as 0.0: the group problem, today's path. ValueError for a value outside [0, 1] or
    NaN, for a ratio without ``groups`` / ``weights`` (``gw`` is :func:`check_groups`' pair) and for a
    non-zero ratio together with ``fit_intercept``, which the sparse-group guard does not cover."""
    if row_ratio is None:
        return 0.0
    tau = float(row_ratio)
    if not 0.0 <= tau <= 1.0:   # (NaN fails both comparisons)
        raise ValueError("row_ratio must be in [0, 1], got %r" % (row_ratio,))
    if gw is None:
        raise ValueError("row_ratio goes with groups and/or weights (without them the penalty is the row norm)")
    if tau > 0.0 and fit_intercept:
        raise ValueError("fit_intercept=True with a non-zero row_ratio is not supported: the intercept guard's "
                         "slack has no sparse-group derivation yet")
    return tau


def check_sample_weight(sample_weight, m: int, dtype=np.float64, name: str = "sample_weight"):
    """The host-side check of observation weights for an m-row A, before any device work. None stays
    None (the unweighted problem, today's path and bits); anything else must be m finite values >= 0
    with at least one > 0 and comes back as a contiguous NumPy array rounded ONCE to ``dtype`` (A's), so
    that every kernel and the guard see the same problem. ValueError for a wrong length, a negative,
    NaN or infinite weight (also one that rounding to float32 makes infinite) and all-zero weights."""
    if sample_weight is None:
        return None
    if isinstance(sample_weight, torch.Tensor):
        sample_weight = sample_weight.detach().cpu().numpy()
    w = np.asarray(sample_weight, dtype=np.float64)
    if w.ndim != 1 or w.size != int(m):
        raise ValueError("%s must have one entry per row of A (%d), got shape %s" % (name, int(m), tuple(w.shape)))
    with np.errstate(over="ignore"):
        w = np.ascontiguousarray(w.astype(np.float32 if np.dtype(dtype) == np.float32 else np.float64))
    if not np.all(np.isfinite(w)):
        raise ValueError("every %s must be finite" % name)
    if np.any(w < 0.0):
        raise ValueError("every %s must be >= 0" % name)
    if not np.any(w > 0.0):
        raise ValueError("%s: at least one weight must be > 0" % name)
    return w


def _np_dtype(A):
    return np.float32 if _dtype_of(A) == torch.float32 else np.float64


def _rows_of(A) -> int:
    return int(np.shape(A)[0]) if len(np.shape(A)) == 2 else -1


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


def _sw_device(w, device):
    """The checked host weights (check_sample_weight) as a device tensor of their own dtype; None stays None."""
    return None if w is None else torch.from_numpy(w).to(device)


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


def _record_sw(xd, Ad, bd, mu: float, fused: int, row_norms: bool, sw, hw=None):
    m, n = Ad.shape
    l = xd.shape[1]
    device = Ad.device
    gdt = _lib.GLX_F64 if Ad.dtype == torch.float64 else _lib.GLX_F32
    rec = (ctypes.c_double * 8)()
    hs = ctypes.c_double(0.0)
    with torch.cuda.device(device):
        nb = ctypes.c_size_t(0)
        check(lib().glx_certificate_sw_workspace_bytes(gdt, m, n, l, ctypes.byref(nb)))
        ws = torch.empty(int(nb.value), dtype=torch.uint8, device=device)
        rn = torch.empty(n, dtype=torch.float64, device=device) if row_norms else None
        check(lib().glx_certificate_sw(gdt, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), float(mu),
                                       int(fused), sw.data_ptr(), None if hw is None else hw.data_ptr(), None,
                                       None if rn is None else rn.data_ptr(), rec, ctypes.byref(hs),
                                       ws.data_ptr(), ws.numel(),
                                       ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    buf = ctypes.create_string_buffer(2048)
    check(lib().glx_certificate_sw_describe(gdt, m, n, l, int(fused), buf, len(buf)))
    return list(rec), rn, buf.value.decode(), float(hs.value)


def _group_record_sw(xd, Ad, bd, mu: float, gw, norms: bool, sw, hw=None):
    ptr, w = gw
    m, n = Ad.shape
    l = xd.shape[1]
    G = int(w.size)
    device = Ad.device
    gdt = _lib.GLX_F64 if Ad.dtype == torch.float64 else _lib.GLX_F32
    rec = (ctypes.c_double * 8)()
    hs = ctypes.c_double(0.0)
    with torch.cuda.device(device):
        nb = ctypes.c_size_t(0)
        check(lib().glx_group_certificate_sw_workspace_bytes(gdt, m, n, l, G, ctypes.byref(nb)))
        ws = torch.empty(int(nb.value), dtype=torch.uint8, device=device)
        gn = torch.empty(G, dtype=torch.float64, device=device) if norms else None
        check(lib().glx_group_certificate_sw(gdt, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), float(mu),
                                             G, ptr.ctypes.data, w.ctypes.data, sw.data_ptr(),
                                             None if hw is None else hw.data_ptr(), None,
                                             None if gn is None else gn.data_ptr(), rec, ctypes.byref(hs),
                                             ws.data_ptr(), ws.numel(),
                                             ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    buf = ctypes.create_string_buffer(2048)
    check(lib().glx_group_certificate_sw_describe(gdt, m, n, l, int(np.diff(ptr).max()), buf, len(buf)))
    return list(rec), gn, buf.value.decode(), float(hs.value)


def _sigma(sw, m: int) -> float:
    """sigma = sum_j w_j on the host in float64, from the weights as rounded to A's dtype (m without)."""
    return float(m) if sw is None else float(np.sum(sw, dtype=np.float64))


def _record_ic(xd, Ad, bd, mu: float, fused: int, norms: bool, sw, sigma: float, hw=None, gw=None):
    """glx_certificate_ic / glx_group_certificate_ic (``gw``): the record of the problem with an intercept,
    (rec, norms, plan, holdout_sum, intercept (l float64))."""
    m, n = Ad.shape
    l = xd.shape[1]
    device = Ad.device
    gdt = _lib.GLX_F64 if Ad.dtype == torch.float64 else _lib.GLX_F32
    rec = (ctypes.c_double * 8)()
    hs = ctypes.c_double(0.0)
    icpt = (ctypes.c_double * l)()
    swp = None if sw is None else sw.data_ptr()
    hwp = None if hw is None else hw.data_ptr()
    buf = ctypes.create_string_buffer(2048)
    with torch.cuda.device(device):
        nb = ctypes.c_size_t(0)
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        if gw is None:
            check(lib().glx_certificate_ic_workspace_bytes(gdt, m, n, l, ctypes.byref(nb)))
            ws = torch.empty(int(nb.value), dtype=torch.uint8, device=device)
            rn = torch.empty(n, dtype=torch.float64, device=device) if norms else None
            check(lib().glx_certificate_ic(gdt, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), float(mu),
                                           int(fused), swp, hwp, float(sigma), None,
                                           None if rn is None else rn.data_ptr(), rec, ctypes.byref(hs), icpt,
                                           ws.data_ptr(), ws.numel(), stream))
            check(lib().glx_certificate_ic_describe(gdt, m, n, l, int(fused), buf, len(buf)))
        else:
            ptr, w = gw
            G = int(w.size)
            check(lib().glx_group_certificate_ic_workspace_bytes(gdt, m, n, l, G, ctypes.byref(nb)))
            ws = torch.empty(int(nb.value), dtype=torch.uint8, device=device)
            rn = torch.empty(G, dtype=torch.float64, device=device) if norms else None
            check(lib().glx_group_certificate_ic(gdt, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), float(mu),
                                                 G, ptr.ctypes.data, w.ctypes.data, swp, hwp, float(sigma), None,
                                                 None if rn is None else rn.data_ptr(), rec, ctypes.byref(hs), icpt,
                                                 ws.data_ptr(), ws.numel(), stream))
            check(lib().glx_group_certificate_ic_describe(gdt, m, n, l, int(np.diff(ptr).max()), buf, len(buf)))
    return list(rec), rn, buf.value.decode(), float(hs.value), np.array(list(icpt), dtype=np.float64)


def compose_groups(rec, mu: float) -> Dict[str, Any]:
    """:func:`compose` for the group certificate's record [||r||^2, <r, b>, sum_g w_g ||x_[g]||,
    max_g ||g_[g]|| / w_g, kkt_max, sum_g kkt_g^2, nonzero groups, 0]: the same arithmetic,
    ``nonzero_groups`` in place of ``nonzero_rows``."""
    out = compose(rec, mu)
    out["nonzero_groups"] = out.pop("nonzero_rows")
    return out


def _group_record(xd: torch.Tensor, Ad: torch.Tensor, bd: torch.Tensor, mu: float, gw, norms: bool):
    ptr, w = gw
    m, n = Ad.shape
    l = xd.shape[1]
    G = int(w.size)
    device = Ad.device
    gdt = _lib.GLX_F64 if Ad.dtype == torch.float64 else _lib.GLX_F32
    rec = (ctypes.c_double * 8)()
    with torch.cuda.device(device):
        nb = ctypes.c_size_t(0)
        check(lib().glx_group_certificate_workspace_bytes(gdt, m, n, l, G, ctypes.byref(nb)))
        ws = torch.empty(int(nb.value), dtype=torch.uint8, device=device)
        gn = torch.empty(G, dtype=torch.float64, device=device) if norms else None
        check(lib().glx_group_certificate(gdt, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), float(mu), G,
                                          ptr.ctypes.data, w.ctypes.data, None,
                                          None if gn is None else gn.data_ptr(), rec, ws.data_ptr(), ws.numel(),
                                          ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    return list(rec), gn, _lib.group_certificate_describe(gdt, m, n, l, int(np.diff(ptr).max()))


def compose_sgl(rec, mu: float, row_ratio: float) -> Dict[str, Any]:
    """:func:`compose_groups` for the sparse-group record (glx_sgl_certificate's 12 values): rec[3] is
    mu / min_g s_g, so the scale composes as before; ``nonzero_rows`` (rec[7]) stands beside
    ``nonzero_groups``, ``fused`` is False, ``scale_min`` is the unclamped min_g s_g and ``row_norm_max``
    max_i ||g_i||."""
    rec = [float(v) for v in rec]
    nzr = rec[7]
    out = compose_groups(rec[:7] + [0.0], mu)
    out["nonzero_rows"] = nzr if math.isnan(nzr) else int(nzr)
    out["row_ratio"] = float(row_ratio)
    out["scale_min"] = rec[8]
    out["row_norm_max"] = rec[10]
    return out


def _sgl_record(xd, Ad, bd, mu: float, tau: float, gw, norms: bool, sw=None, hw=None):
    """glx_sgl_certificate_sw: (rec (12), row norms (n) or None, plan, holdout_sum)."""
    ptr, w = gw
    m, n = Ad.shape
    l = xd.shape[1]
    G = int(w.size)
    device = Ad.device
    gdt = _lib.GLX_F64 if Ad.dtype == torch.float64 else _lib.GLX_F32
    rec = (ctypes.c_double * 12)()
    hs = ctypes.c_double(0.0)
    with torch.cuda.device(device):
        nb = ctypes.c_size_t(0)
        check(lib().glx_sgl_certificate_workspace_bytes(gdt, m, n, l, G, ctypes.byref(nb)))
        ws = torch.empty(int(nb.value), dtype=torch.uint8, device=device)
        rn = torch.empty(n, dtype=torch.float64, device=device) if norms else None
        check(lib().glx_sgl_certificate_sw(gdt, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), float(mu),
                                           float(tau), G, ptr.ctypes.data, w.ctypes.data,
                                           None if sw is None else sw.data_ptr(),
                                           None if hw is None else hw.data_ptr(), None,
                                           None if rn is None else rn.data_ptr(), rec, ctypes.byref(hs),
                                           ws.data_ptr(), ws.numel(),
                                           ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    buf = ctypes.create_string_buffer(2048)
    check(lib().glx_sgl_certificate_describe(gdt, m, n, l, int(sw is not None), buf, len(buf)))
    return list(rec), rn, buf.value.decode(), float(hs.value)


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


def certificate(x, A, b, mu, groups=None, weights=None, *, fused: int = 0, row_norms: bool = False,
                sample_weight=None, fit_intercept: bool = False, row_ratio=None) -> Dict[str, Any]:
    """The duality gap and KKT violation of the iterate ``x`` at ``mu`` (module docstring).

    ``row_ratio`` (None or 0: today's group path, call for call; needs ``groups`` / ``weights``): tau in
    [0, 1], the certificate of the sparse-group penalty ``mu (tau sum_i ||x_i||_2 + (1 - tau) sum_g w_g
    ||x_[g]||_F)`` (DESIGN.md "Sparse-group lasso"). The dual point is ``s r`` with ``s = min(1, min_g s_g)``,
    ``s_g`` the largest scaling at which group g's constraint ``||S_a((A^T theta)_[g])||_F <= c_g`` holds
    (a = tau mu, c_g = (1 - tau) mu w_g, S_a the row-wise shrinkage). The result carries the group keys plus
    ``row_ratio``, ``nonzero_rows``, ``scale_min`` and ``row_norm_max``; ``gmax`` is ``mu / min_g s_g`` and
    ``row_norms=True`` returns ``row_norms``, ||g_i|| of the n rows. It composes with ``sample_weight``;
    with ``fit_intercept=True`` it raises ValueError.

    ``x`` (n x l), ``A`` (m x n) and ``b`` (m x l) are NumPy arrays or torch tensors and are not
    modified; the computation runs in A's dtype. ``fused``: 0 auto, 1 the row terms in the epilogue of
    A^T r where the plan admits it, 2 a row kernel behind the plain product (the same bits). Returns
    ``primal``, ``dual``, ``gap`` (>= primal - min P up to rounding), ``rel_gap`` = gap /
    max(|primal|, tiny), ``scale`` (s), ``gmax``, ``kkt_max``, ``kkt_fro``, ``nonzero_rows``,
    ``fused`` (whether the fused form ran), ``plan`` (glx_certificate_describe's line) and, with
    ``row_norms=True``, ``row_norms``: ||g_i||_2 for every row, a float64 array of length n (NumPy
    for NumPy inputs, a device tensor otherwise).

    ``groups`` / ``weights`` (module docstring; both None: the row problem, today's path and bits):
    the certificate of ``mu sum_g w_g ||x_[g]||_F``. ``nonzero_groups`` replaces ``nonzero_rows``,
    ``gmax`` is ``max_g ||g_[g]|| / w_g``, ``fused`` is False (the group terms run behind the plain
    product) and ``row_norms=True`` returns ``group_norms``: ``||g_[g]|| / w_g``, length G.

    ``sample_weight`` (None: today's path, bit for bit): m observation weights ``w_j >= 0``, the
    certificate of ``1/2 sum_j w_j ||(A x - b)_j||^2 + mu Omega(x)`` (:func:`check_sample_weight`; it
    composes with ``groups`` / ``weights``, which weigh features). A is neither copied nor scaled.

    ``fit_intercept`` (False: today's path, call for call): the certificate of
    ``min_c 1/2 sum_j w_j ||(A x + 1 c^T - b)_j||^2 + mu Omega(x)`` with an unpenalised intercept c in R^l
    (DESIGN.md "Intercept"). c is eliminated exactly: ``intercept`` (l float64 values) is minus the
    weighted column mean of A x - b, ``primal``, ``dual``, ``gap`` and ``rel_gap`` speak of the minimum
    over c, and ``gmax`` / the row norms are those of A^T (w o r_c) with r_c the centred residual. It
    composes with ``groups`` / ``weights`` and ``sample_weight``; A is not centred."""
    mu = float(mu)
    if not mu >= 0.0:
        raise ValueError("mu must be >= 0")
    gw = check_groups(groups, weights, np.shape(A)[1] if len(np.shape(A)) == 2 else -1,
                      np.shape(b)[1] if len(np.shape(b)) == 2 else 1)
    tau = check_row_ratio(row_ratio, gw, fit_intercept)
    sw = check_sample_weight(sample_weight, _rows_of(A), _np_dtype(A))
    xd, Ad, bd = _inputs(x, A, b)
    swd = _sw_device(sw, Ad.device)
    if tau > 0.0:
        rec, rn, plan, _ = _sgl_record(xd, Ad, bd, mu, tau, gw, row_norms, swd)
        out = compose_sgl(rec, mu, tau)
        out["plan"] = plan
        if row_norms:
            out["row_norms"] = rn if isinstance(A, torch.Tensor) else rn.cpu().numpy()
        return out
    if fit_intercept:
        rec, nrm, plan, _, icpt = _record_ic(xd, Ad, bd, mu, fused, row_norms, swd, _sigma(sw, Ad.shape[0]), None, gw)
        out = compose(rec, mu) if gw is None else compose_groups(rec, mu)
        out["plan"] = plan
        out["intercept"] = icpt
        if row_norms:
            key = "row_norms" if gw is None else "group_norms"
            out[key] = nrm if isinstance(A, torch.Tensor) else nrm.cpu().numpy()
        return out
    if gw is not None:
        if swd is not None:
            rec, gn, plan, _ = _group_record_sw(xd, Ad, bd, mu, gw, row_norms, swd)
        else:
            rec, gn, plan = _group_record(xd, Ad, bd, mu, gw, row_norms)
        out = compose_groups(rec, mu)
        out["plan"] = plan
        if row_norms:
            out["group_norms"] = gn if isinstance(A, torch.Tensor) else gn.cpu().numpy()
        return out
    if swd is not None:
        rec, rn, plan, _ = _record_sw(xd, Ad, bd, mu, fused, row_norms, swd)
    else:
        rec, rn, plan = _record(xd, Ad, bd, mu, fused, row_norms)
    out = compose(rec, mu)
    out["plan"] = plan
    if row_norms:
        out["row_norms"] = rn if isinstance(A, torch.Tensor) else rn.cpu().numpy()
    return out


def mu_max(A, b, groups=None, weights=None, sample_weight=None, fit_intercept: bool = False,
           row_ratio=None) -> float:
    """The smallest mu for which x = 0 is optimal, max_i ||(A^T b)_i||_2: the certificate's gmax at
    x = 0, where r = -b. With ``groups`` / ``weights``: max_g ||(A^T b)_[g]||_F / w_g. With
    ``sample_weight``: of A^T W b. With ``fit_intercept``: of A^T W (b - 1 b-bar^T), b-bar the weighted
    column mean of b (at and above it the solution is x = 0 with the intercept b-bar). With ``row_ratio``
    (tau > 0, the sparse-group penalty): 1 / min_g s_g from the dual-scale launch on g = A^T b at mu = 1."""
    gw = check_groups(groups, weights, np.shape(A)[1] if len(np.shape(A)) == 2 else -1,
                      np.shape(b)[1] if len(np.shape(b)) == 2 else 1)
    tau = check_row_ratio(row_ratio, gw, fit_intercept)
    sw = check_sample_weight(sample_weight, _rows_of(A), _np_dtype(A))
    xd, Ad, bd = _inputs(None, A, b)
    if tau > 0.0:
        smin = _sgl_record(xd, Ad, bd, 1.0, tau, gw, False, _sw_device(sw, Ad.device))[0][8]
        return 1.0 / smin if smin > 0.0 else float("inf")
    if fit_intercept:
        return float(_record_ic(xd, Ad, bd, 0.0, 0, False, _sw_device(sw, Ad.device), _sigma(sw, Ad.shape[0]), None,
                                gw)[0][3])
    if sw is not None:
        swd = _sw_device(sw, Ad.device)
        if gw is not None:
            return float(_group_record_sw(xd, Ad, bd, 0.0, gw, False, swd)[0][3])
        return float(_record_sw(xd, Ad, bd, 0.0, 0, False, swd)[0][3])
    if gw is not None:
        return float(_group_record(xd, Ad, bd, 0.0, gw, False)[0][3])
    rec, _, _ = _record(xd, Ad, bd, 0.0, 0, False)
    return float(rec[3])
