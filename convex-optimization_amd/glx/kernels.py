"""Single-kernel entry points of libglx (``glx_residual`` / ``glx_gradient`` / ``glx_prox`` /
``glx_residual_gradient``).

These are the dense products and the group prox of the reference iteration exposed one at a
time — ``A @ x - b`` (gl_ProxGD_primal.py:25,61), ``A.T @ r`` (:129) and ``prox_th``
(:65-71) — used by the kernel-level tests and available for composition, and one line-search
trial at a time (``glx_trial_proxgd`` / ``glx_trial_fista``: the row kernels, the A^T R epilogues
and the replicated halves of the row-sharded schedules), and the descent-method kernels one
launch at a time (``glx_descent_step``, ``glx_fgd_gradient``, ``glx_row_stats``,
``glx_threshold``, ``glx_thr_combine``, ``glx_descent_pass``), and the dual ADMM solver's row step,
Gram kernel and host eigenvalue sweep (``glx_admm_dual_step``, ``glx_admm_primal_step``, ``glx_gram``,
``glx_sym_lambda_max``), and the dual ALM solver's inner step and inner loop (``glx_alm_inner_step``,
``glx_alm_inner_run``), and the three splitting solvers' glue kernels (``glx_admm_rhs``, ``glx_admm_fin``,
``glx_admm_primal_rhs``, ``glx_admm_primal_fin``, ``glx_alm_j``, ``glx_alm_x``), and the optimality certificate's row terms (``glx_certificate_step``), and
the split-candidate trial's dense pass with A e fused in, one launch (``glx_fused_ae_pass``, ``glx_dense_pass_keep``), and
the pieces of gap-safe screening (``glx_col_norms``, ``glx_screen_step``, ``glx_gather_cols`` and the
host-only ``glx_screen_guard``). All
tensors are contiguous device
tensors of one dtype (float32 / float64).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import check, lib


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float64:
        return _lib.GLX_F64
    if t.dtype == torch.float32:
        return _lib.GLX_F32
    raise ValueError("float32 or float64 required")


def _ws(dtype: int, m: int, n: int, l: int, device) -> torch.Tensor:
    nb = ctypes.c_size_t(0)
    check(lib().glx_kernel_workspace_bytes(dtype, m, n, l, ctypes.byref(nb)))
    return torch.empty(int(nb.value), dtype=torch.uint8, device=device)


def _trial_ws(dtype: int, m: int, n: int, l: int, device) -> torch.Tensor:
    nb = ctypes.c_size_t(0)
    check(lib().glx_trial_workspace_bytes(dtype, m, n, l, ctypes.byref(nb)))
    return torch.empty(int(nb.value), dtype=torch.uint8, device=device)


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def residual(A: torch.Tensor, X: torch.Tensor, B: torch.Tensor, variant: int = 0
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """R = A X - B and 1/2 ||R||_F^2 (a 1-element float64 device tensor)."""
    m, n = A.shape
    l = X.shape[1]
    dt = _dt(A)
    R = torch.empty((m, l), dtype=A.dtype, device=A.device)
    h = torch.empty(1, dtype=torch.float64, device=A.device)
    ws = _ws(dt, m, n, l, A.device)
    check(lib().glx_residual(dt, m, n, l, A.data_ptr(), X.data_ptr(), B.data_ptr(), R.data_ptr(),
                             h.data_ptr(), ws.data_ptr(), ws.numel(), variant, _stream(A.device)))
    return R, h


def residual_batch(A: torch.Tensor, Xs, B: torch.Tensor, variant: int = 0):
    """R_i = A X_i - B for up to three right-hand sides in one pass over A; also returns the
    squared norms ||R_i||^2 (float64 device tensor)."""
    m, n = A.shape
    l = Xs[0].shape[1]
    dt = _dt(A)
    Rs = [torch.empty((m, l), dtype=A.dtype, device=A.device) for _ in Xs]
    sq = torch.empty(4, dtype=torch.float64, device=A.device)
    ws = _ws(dt, m, n, l, A.device)
    xp = (ctypes.c_void_p * 3)(*[x.data_ptr() for x in Xs], *([None] * (3 - len(Xs))))
    rp = (ctypes.c_void_p * 3)(*[r.data_ptr() for r in Rs], *([None] * (3 - len(Rs))))
    check(lib().glx_residual_batch(dt, m, n, l, A.data_ptr(), len(Xs), xp, B.data_ptr(), rp,
                                   sq.data_ptr(), ws.data_ptr(), ws.numel(), variant,
                                   _stream(A.device)))
    return Rs, sq


def gradient(A: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    """G = A^T R."""
    m, n = A.shape
    l = R.shape[1]
    dt = _dt(A)
    G = torch.empty((n, l), dtype=A.dtype, device=A.device)
    ws = _ws(dt, m, n, l, A.device)
    check(lib().glx_gradient(dt, m, n, l, A.data_ptr(), R.data_ptr(), G.data_ptr(), ws.data_ptr(),
                             ws.numel(), _stream(A.device)))
    return G


def residual_gradient(A: torch.Tensor, X: torch.Tensor, B: torch.Tensor, one_pass: bool = False
                      ) -> Tuple[torch.Tensor, torch.Tensor, bool]:
    """R = A X - B and G = A^T R: two passes over A (the faster path), or with one_pass=True
    the fused kernel that reads A from HBM once, where the shape and device allow it.
    Returns (R, G, one_pass_ran)."""
    m, n = A.shape
    l = X.shape[1]
    dt = _dt(A)
    R = torch.empty((m, l), dtype=A.dtype, device=A.device)
    G = torch.empty((n, l), dtype=A.dtype, device=A.device)
    ws = _ws(dt, m, n, l, A.device)
    fused = ctypes.c_int(0)
    check(lib().glx_residual_gradient(dt, m, n, l, A.data_ptr(), X.data_ptr(), B.data_ptr(),
                                      R.data_ptr(), G.data_ptr(), ws.data_ptr(), ws.numel(),
                                      1 if one_pass else 0, ctypes.byref(fused), _stream(A.device)))
    return R, G, bool(fused.value)


def residual_gradient2(A: torch.Tensor, X0: torch.Tensor, X1: torch.Tensor, B: torch.Tensor,
                       one_pass: bool = True
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, bool]:
    """The line-search trial's batch and the next gradient: R0 = A X0 - B, R1 = A X1 - B and
    G = A^T R1, with one read of A (the l = 16 role-split kernel) where the shape and device
    allow it, else A @ [X0 | X1] then A^T R1. Returns (R0, R1, G, one_pass_ran)."""
    m, n = A.shape
    l = X0.shape[1]
    dt = _dt(A)
    R0 = torch.empty((m, l), dtype=A.dtype, device=A.device)
    R1 = torch.empty((m, l), dtype=A.dtype, device=A.device)
    G = torch.empty((n, l), dtype=A.dtype, device=A.device)
    ws = _ws(dt, m, n, l, A.device)
    ran = ctypes.c_int(0)
    check(lib().glx_residual_gradient2(dt, m, n, l, A.data_ptr(), X0.data_ptr(), X1.data_ptr(),
                                       B.data_ptr(), R0.data_ptr(), R1.data_ptr(), G.data_ptr(),
                                       ws.data_ptr(), ws.numel(), 1 if one_pass else 0,
                                       ctypes.byref(ran), _stream(A.device)))
    return R0, R1, G, bool(ran.value)


def flagged_rows_product(At: torch.Tensor, E: torch.Tensor, row_masks: torch.Tensor,
                         form: int = 0) -> torch.Tensor:
    """Y = sum over the rows k with row_masks[k] != 0 of At[k]^T E[k] (m x l): the split-candidate
    trial's A e from the transposed copy At = A^T (n x m). form 0: the MFMA row form
    (m % 64 == 0), 1: the VALU column-list gather of rounds 2-4, 2: the bitmap gather (the
    solver's default; 1 and 2 need bit c of row_masks[k] == (E[k][c] != 0)). row_masks: int32
    device tensor of n (+ padding) column masks."""
    n, m = At.shape
    l = E.shape[1]
    dt = _dt(At)
    Y = torch.empty((m, l), dtype=At.dtype, device=At.device)
    ws = _ws(dt, m, n, l, At.device)
    check(lib().glx_flagged_rows_product(dt, m, n, l, At.data_ptr(), E.data_ptr(),
                                         row_masks.data_ptr(), Y.data_ptr(), int(form),
                                         ws.data_ptr(), ws.numel(), _stream(At.device)))
    return Y


def fused_ae_pass(A: torch.Tensor, p: torch.Tensor, thres: float = 1e-3) -> Dict[str, object]:
    """The split-candidate trial's dense pass with A e fused in, one launch (glx_fused_ae_pass;
    float64, where the shape's one-source plan under GLX_AX_VARIANT / GLX_AX_S is the LDS-DMA tile
    92278). e = p - thr(p); its row masks and column bitmaps come from the trial's own replicated
    half (trial_proxgd form 2, emode), in the layout include/glx.h documents for zf. Returns a
    dict with P (S, m, l: A p per K split), Pe (S, m, l: A e per K split), S, rotated (the chunk
    rotation of GLX_AX_ROT is on), e and zf."""
    m, n = A.shape
    l = p.shape[1]
    if A.dtype != torch.float64 or p.dtype != torch.float64:
        raise ValueError("float64 required")
    S, rot = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().glx_fused_ae_pass(m, n, l, None, None, None, None, None, ctypes.byref(S),
                                  ctypes.byref(rot), None))
    tr = trial_proxgd(p, None, 1.0, 0.0, thres=thres, form=2, emode=True, p=p)
    P = torch.full((S.value, m, l), float("nan"), dtype=A.dtype, device=A.device)
    Pe = torch.full((S.value, m, l), float("nan"), dtype=A.dtype, device=A.device)
    check(lib().glx_fused_ae_pass(m, n, l, A.data_ptr(), p.data_ptr(), tr["zf"].data_ptr(),
                                  P.data_ptr(), Pe.data_ptr(), ctypes.byref(S), ctypes.byref(rot),
                                  _stream(A.device)))
    return {"P": P, "Pe": Pe, "S": int(S.value), "rotated": bool(rot.value), "e": tr["z"],
            "zf": tr["zf"]}


def dense_pass_keep(A: torch.Tensor, p: torch.Tensor, keep_mib: int, fused: bool = True,
                    thres: float = 1e-3) -> Dict[str, object]:
    """The dense pass of :func:`fused_ae_pass` alone with a given Infinity-Cache keep size
    (glx_dense_pass_keep): about ``keep_mib`` MiB of A, the last chunks of every block's walk, load
    with the default policy, the rest non-temporally (0: all non-temporal, as fused_ae_pass).
    ``fused``: the launch with A e fused in; else the plain launch of the same tile (Pe, e, zf are
    None). Returns the dict of fused_ae_pass."""
    m, n = A.shape
    l = p.shape[1]
    if A.dtype != torch.float64 or p.dtype != torch.float64:
        raise ValueError("float64 required")
    S, rot = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().glx_dense_pass_keep(m, n, l, None, None, None, None, None, int(keep_mib),
                                    ctypes.byref(S), ctypes.byref(rot), None))
    tr = trial_proxgd(p, None, 1.0, 0.0, thres=thres, form=2, emode=True, p=p) if fused else None
    P = torch.full((S.value, m, l), float("nan"), dtype=A.dtype, device=A.device)
    Pe = torch.full((S.value, m, l), float("nan"), dtype=A.dtype, device=A.device) if fused else None
    check(lib().glx_dense_pass_keep(m, n, l, A.data_ptr(), p.data_ptr(),
                                    tr["zf"].data_ptr() if fused else None, P.data_ptr(), _ptr(Pe),
                                    int(keep_mib), ctypes.byref(S), ctypes.byref(rot), _stream(A.device)))
    return {"P": P, "Pe": Pe, "S": int(S.value), "rotated": bool(rot.value),
            "e": tr["z"] if fused else None, "zf": tr["zf"] if fused else None}


def trial_mask_words(n: int) -> int:
    """uint32 words of a trial's zf buffer for n rows (glx_trial_mask_bytes): the padded row masks,
    then the column bitmaps (layout in include/glx.h)."""
    nb = ctypes.c_size_t(0)
    check(lib().glx_trial_mask_bytes(int(n), ctypes.byref(nb)))
    return int(nb.value) // 4


def _zf_arg(zf: Optional[torch.Tensor], want: bool, n: int, device) -> Optional[torch.Tensor]:
    if zf is None and want:
        zf = torch.zeros(trial_mask_words(n), dtype=torch.int32, device=device)
    if zf is not None and (zf.dtype != torch.int32 or zf.numel() < trial_mask_words(n)):
        raise ValueError("zf must be an int32 tensor of trial_mask_words(n) words")
    return zf


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def trial_proxgd(x: torch.Tensor, G: Optional[torch.Tensor], t: float, mu: float,
                 thres: float = 1e-3, form: int = 0, emode: bool = False,
                 A: Optional[torch.Tensor] = None, R: Optional[torch.Tensor] = None,
                 p: Optional[torch.Tensor] = None, zf: Optional[torch.Tensor] = None
                 ) -> Dict[str, Optional[torch.Tensor]]:
    """One ProxGD line-search trial (glx_trial_proxgd). form 0: the row kernel on the given G;
    form 1: the epilogue of G = A^T R (A, R given, G returned); form 2: the replicated half of the
    row-sharded schedule from a given p (x = the thresholded iterate). emode: z holds
    e = p - pthr and zf (int32 words, bit patterns of uint32; allocated zeroed unless passed in:
    the kernels do not clear it) the masks and column bitmaps of e. Returns a dict with G, p,
    pthr, z, sums (6 float64; None in form 2) and zf (None where not written)."""
    n, l = x.shape
    dt = _dt(x)
    dev = x.device
    m = A.shape[0] if form == 1 else 1
    new = lambda: torch.empty((n, l), dtype=x.dtype, device=dev)  # noqa: E731
    if form == 1:
        G = new()
    if form != 2:
        p = new()
    pthr, z = new(), new()
    sums = None if form == 2 else torch.full((6,), float("nan"), dtype=torch.float64, device=dev)
    zf = _zf_arg(zf, bool(emode), n, dev)
    ws = _trial_ws(dt, m, n, l, dev)
    check(lib().glx_trial_proxgd(dt, m, n, l, _ptr(A), _ptr(R), _ptr(G), x.data_ptr(), float(t),
                                 float(mu), float(thres), int(form), 1 if emode else 0,
                                 p.data_ptr(), pthr.data_ptr(), z.data_ptr(), _ptr(sums), _ptr(zf),
                                 ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"G": G, "p": p, "pthr": pthr, "z": z, "sums": sums, "zf": zf}


def fin_atr_prox(A: torch.Tensor, P: torch.Tensor, B: torch.Tensor, x: torch.Tensor, t: float, mu: float,
                 S: int, S0: int = 0, chain: int = 0, cx: Optional[torch.Tensor] = None,
                 cmax: Optional[torch.Tensor] = None, cmax_parts: Optional[torch.Tensor] = None,
                 thres: float = 1e-3, emode: bool = False, head: bool = True
                 ) -> Dict[str, Optional[torch.Tensor]]:
    """A residual finalize and the fused A^T R + ProxGD trial behind it (glx_fin_atr_prox; float64).
    P: the slabs ((S0 + S, m, l) with a chain, else (2 S, m, l): source 0 then source 1). head=False:
    k_finalize_residual then k_atr_prox; head=True: one launch with the finalize at the head of
    k_atr_prox. cx: the count's array (n, l) with cmax (1 float64) or cmax_parts ((np, 6) float64
    trial partials, the max of column 3). Returns a dict with R0, R1, fin_parts ((blocks, 4)), G, p,
    pthr, z, sums (6) and zf."""
    m, n = A.shape
    l = x.shape[1]
    if A.dtype != torch.float64:
        raise ValueError("float64 required")
    dev = A.device
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)  # noqa: E731
    R0, R1 = nan(m, l), nan(m, l)
    G, p, pthr, z = nan(n, l), nan(n, l), nan(n, l), nan(n, l)
    parts = nan(1024, 4)
    sums = nan(6)
    zf = _zf_arg(None, bool(emode), n, dev)
    hws = torch.zeros(8192, dtype=torch.uint8, device=dev)
    ws = _trial_ws(_lib.GLX_F64, m, n, l, dev)
    nb = ctypes.c_int(0)
    check(lib().glx_fin_atr_prox(m, n, l, A.data_ptr(), P.data_ptr(), int(S), int(S0), int(chain),
                                 B.data_ptr(), R0.data_ptr(), R1.data_ptr(), _ptr(cx), _ptr(cmax),
                                 _ptr(cmax_parts), 0 if cmax_parts is None else int(cmax_parts.shape[0]),
                                 parts.data_ptr(), ctypes.byref(nb), G.data_ptr(), x.data_ptr(), float(t),
                                 float(mu), float(thres), 1 if emode else 0, p.data_ptr(), pthr.data_ptr(),
                                 z.data_ptr(), sums.data_ptr(), _ptr(zf), 1 if head else 0, hws.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"R0": R0, "R1": R1, "fin_parts": parts[:nb.value], "G": G, "p": p, "pthr": pthr, "z": z,
            "sums": sums, "zf": zf}


def trial_fista(y: Optional[torch.Tensor], G: Optional[torch.Tensor], xk: torch.Tensor, t: float,
                mu: float, theta: float, theta_next: float, thres: float = 1e-3,
                delta: float = 0.0, form: int = 0, prox: bool = True, split: bool = False,
                A: Optional[torch.Tensor] = None, R: Optional[torch.Tensor] = None,
                xc: Optional[torch.Tensor] = None, zf: Optional[torch.Tensor] = None
                ) -> Dict[str, Optional[torch.Tensor]]:
    """One FProxGD (prox) / FGD trial with the next combine (glx_trial_fista). form 0: the row
    kernel on the given G; form 1: the epilogue of G = A^T R; form 2: the replicated half from a
    given xc (y, G unused). split: also ec = xc - thr(xc) and zf, its masks and column bitmaps (as
    trial_proxgd). Returns a dict with G, xc, vnext, ynext, ec, sums (4 float64, FGD 5; None in
    form 2) and zf."""
    n, l = xk.shape
    dt = _dt(xk)
    dev = xk.device
    m = A.shape[0] if form == 1 else 1
    new = lambda: torch.empty((n, l), dtype=xk.dtype, device=dev)  # noqa: E731
    if form == 1:
        G = new()
    if form != 2:
        xc = new()
    vnext, ynext = new(), new()
    ec = new() if split else None
    sums = None if form == 2 else torch.full((6,), float("nan"), dtype=torch.float64, device=dev)
    zf = _zf_arg(zf, bool(split), n, dev)
    ws = _trial_ws(dt, m, n, l, dev)
    check(lib().glx_trial_fista(dt, m, n, l, _ptr(A), _ptr(R), _ptr(G), _ptr(y), xk.data_ptr(),
                                float(t), float(mu), float(thres), float(theta), float(theta_next),
                                float(delta), int(form), 1 if prox else 0, xc.data_ptr(),
                                vnext.data_ptr(), ynext.data_ptr(), _ptr(ec), _ptr(sums), _ptr(zf),
                                ws.data_ptr(), ws.numel(), _stream(dev)))
    if sums is not None:
        sums = sums[:4 if prox else 5]
    return {"G": G, "xc": xc, "vnext": vnext, "ynext": ynext, "ec": ec, "sums": sums, "zf": zf}


def _descent_ws(dtype: int, m: int, n: int, l: int, device) -> torch.Tensor:
    nb = ctypes.c_size_t(0)
    check(lib().glx_descent_workspace_bytes(dtype, m, n, l, ctypes.byref(nb)))
    return torch.empty(int(nb.value), dtype=torch.uint8, device=device)


def _nan_sums(k: int, device) -> torch.Tensor:
    return torch.full((k,), float("nan"), dtype=torch.float64, device=device)


def _slabs(g: torch.Tensor, n: int, l: int) -> int:
    if g.dim() == 2:
        if tuple(g.shape) != (n, l):
            raise ValueError("g must be (n, l) or (S, n, l)")
        return 1
    if g.dim() != 3 or tuple(g.shape[1:]) != (n, l) or g.shape[0] < 1:
        raise ValueError("g must be (n, l) or (S, n, l)")
    return int(g.shape[0])


def descent_step(xt: torch.Tensor, g: torch.Tensor, alpha: float, mu: float, thres: float = 1e-3,
                 delta: float = 0.0, mode: int = 0) -> Dict[str, torch.Tensor]:
    """One SGD (mode 0) / GD (mode 1) step (glx_descent_step) from the thresholded iterate xt
    (n x l, left unchanged: the kernel works on a copy) and the gradient g, (n, l) or S slabs
    (S, n, l) summed in slab order. Returns a dict with x = xt - alpha (g + mu xt / d),
    xt = thr(x) and sum (1 float64: sum_i ||x_i||)."""
    n, l = xt.shape
    dt = _dt(xt)
    dev = xt.device
    S = _slabs(g, n, l)
    x = torch.empty_like(xt)
    xt_io = xt.clone()
    s = _nan_sums(1, dev)
    ws = _descent_ws(dt, 1, n, l, dev)
    check(lib().glx_descent_step(dt, n, l, int(mode), g.data_ptr(), S, float(alpha), float(mu),
                                 float(thres), float(delta), x.data_ptr(), xt_io.data_ptr(),
                                 s.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"x": x, "xt": xt_io, "sum": s}


def fgd_gradient(y: torch.Tensor, gp: torch.Tensor, mu: float, delta: float
                 ) -> Dict[str, torch.Tensor]:
    """FGD's smoothed gradient (glx_fgd_gradient): g = sum of gp's slabs + mu y / sqrt(||y_i||^2 +
    delta^2), gp (n, l) or (S, n, l). Returns a dict with g and sum (1 float64: the smoothed
    norm sum_i (sqrt(||y_i||^2 + delta^2) - delta))."""
    n, l = y.shape
    dt = _dt(y)
    dev = y.device
    S = _slabs(gp, n, l)
    g = torch.empty_like(y)
    s = _nan_sums(1, dev)
    ws = _descent_ws(dt, 1, n, l, dev)
    check(lib().glx_fgd_gradient(dt, n, l, y.data_ptr(), gp.data_ptr(), S, float(mu), float(delta),
                                 g.data_ptr(), s.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _stream(dev)))
    return {"g": g, "sum": s}


def row_stats(x: torch.Tensor) -> Dict[str, torch.Tensor]:
    """glx_row_stats: a dict with stats = [sum_i ||x_i||, max |x|, #{|x| > 1e-6 max |x|}]
    (3 float64)."""
    n, l = x.shape
    dt = _dt(x)
    s = _nan_sums(3, x.device)
    ws = _descent_ws(dt, 1, n, l, x.device)
    check(lib().glx_row_stats(dt, n, l, x.data_ptr(), s.data_ptr(), ws.data_ptr(), ws.numel(),
                              _stream(x.device)))
    return {"stats": s}


def threshold(x: torch.Tensor, thres: float, flag: Optional[torch.Tensor] = None, epoch: int = 1,
              inplace: bool = False) -> Dict[str, torch.Tensor]:
    """glx_threshold on the x.numel() values of x: xo = x with |x| < thres zeroed (inplace: x
    itself), flag (1 int32, -1 unless passed in) = epoch when a nonzero value was zeroed."""
    dt = _dt(x)
    xo = x if inplace else torch.empty_like(x)
    if flag is None:
        flag = torch.full((1,), -1, dtype=torch.int32, device=x.device)
    if flag.dtype != torch.int32:
        raise ValueError("flag must be an int32 tensor")
    check(lib().glx_threshold(dt, x.numel(), x.data_ptr(), xo.data_ptr(), float(thres),
                              flag.data_ptr(), int(epoch), _stream(x.device)))
    return {"xo": xo, "flag": flag}


def thr_combine(xk: torch.Tensor, vk: torch.Tensor, thres: float, a: float, b: float
                ) -> Dict[str, torch.Tensor]:
    """glx_thr_combine: a dict with xk = thr(xk) (a copy; the kernel's in-place output) and
    y = a thr(xk) + b vk."""
    dt = _dt(xk)
    xo = xk.clone()
    y = torch.empty_like(xk)
    check(lib().glx_thr_combine(dt, xk.numel(), xo.data_ptr(), vk.data_ptr(), y.data_ptr(),
                                float(thres), float(a), float(b), _stream(xk.device)))
    return {"xk": xo, "y": y}


def descent_pass(A: torch.Tensor, x: torch.Tensor, xt: torch.Tensor, b: torch.Tensor,
                 fh_mu: Optional[float] = None, rn: Optional[torch.Tensor] = None, nt: int = -1,
                 G: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None
                 ) -> Dict[str, object]:
    """One pass over A of an l = 1 descent iteration (glx_descent_pass): G = A^T (A xt - b),
    sums = [sum (A x - b)^2, sum (A xt - b)^2] (2 float64) and, with fh_mu and rn (1 float64
    device value) given, fh = 0.5 sums[0] + fh_mu rn. x, xt of n values, b of m. G and sums are
    allocated (sums filled with NaN) unless passed in. Returns a dict with G, sums, fh (None
    without fh_mu) and blocks, the workgroup count. GlxError (GLX_E_INVALID) where the kernel
    does not apply."""
    m, n = A.shape
    dt = _dt(A)
    dev = A.device
    if x.numel() != n or xt.numel() != n or b.numel() != m:
        raise ValueError("x, xt of n values and b of m")
    if G is None:
        G = torch.empty(n, dtype=A.dtype, device=dev)
    if sums is None:
        sums = _nan_sums(2, dev)
    fh = _nan_sums(1, dev) if fh_mu is not None else None
    nb = ctypes.c_int(0)
    ws = _descent_ws(dt, m, n, 1, dev)
    check(lib().glx_descent_pass(dt, m, n, A.data_ptr(), x.data_ptr(), xt.data_ptr(), b.data_ptr(),
                                 G.data_ptr(), sums.data_ptr(), _ptr(fh),
                                 float(fh_mu) if fh_mu is not None else 0.0, _ptr(rn), int(nt),
                                 ctypes.byref(nb), ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"G": G, "sums": sums, "fh": fh, "blocks": int(nb.value)}


def prox(W: torch.Tensor, t: float, mu: float, thres: float = 1e-3
         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Group prox with the reference's denominator quirk; returns (X, [sum ||x_i||, max|x|])."""
    n, l = W.shape
    dt = _dt(W)
    X = torch.full_like(W, float("nan"))
    sums = _nan_sums(2, W.device)
    ws = _ws(dt, 1, n, l, W.device)
    check(lib().glx_prox(dt, n, l, W.data_ptr(), float(t), float(mu), float(thres), X.data_ptr(),
                         sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream(W.device)))
    return X, sums


def _admm_ws(dtype: int, m: int, n: int, l: int, device) -> torch.Tensor:
    nb = ctypes.c_size_t(0)
    check(lib().glx_admm_workspace_bytes(dtype, m, n, l, None, ctypes.byref(nb)))
    return torch.empty(int(nb.value), dtype=torch.uint8, device=device)


def admm_dual_step(x: torch.Tensor, rho: float, tau: float, mu: float, G: Optional[torch.Tensor] = None,
                   A: Optional[torch.Tensor] = None, Z: Optional[torch.Tensor] = None, form: int = 0,
                   m: int = 1) -> Dict[str, torch.Tensor]:
    """The dual ADMM row step (gl_ADMM_dual.py:64-67, glx_admm_dual_step): w = x / rho - g,
    u = (mu w) / max(||w_i||, mu), r = u + g, x_new = x - (tau rho) r. form 0: the row kernel on
    the given G (with ``m`` the rows of A: on the panel layout a solve's unfused arm takes at
    (m, n, l), bit-identical to form 1; m = 1: the generic row layout); form 1: the epilogue of
    G = A^T Z (G is computed and returned). Returns
    {"G", "u", "x", "r", "sums"} with sums = [sum_i ||x_new_i||, max |x_new|] (float64)."""
    n, l = x.shape
    dt = _dt(x)
    dev = x.device
    if form == 1:
        if A is None or Z is None:
            raise ValueError("form 1 needs A and Z")
        m = A.shape[0]
        G = torch.full((n, l), float("nan"), dtype=x.dtype, device=dev)
    else:
        if G is None:
            raise ValueError("form 0 needs G")
    u = torch.full_like(x, float("nan"))
    xn = torch.full_like(x, float("nan"))
    r = torch.full_like(x, float("nan"))
    sums = _nan_sums(2, dev)
    ws = _admm_ws(dt, m, n, l, dev)
    check(lib().glx_admm_dual_step(dt, m, n, l, _ptr(A), _ptr(Z), G.data_ptr(), x.data_ptr(), float(rho),
                                   float(tau), float(mu), int(form), u.data_ptr(), xn.data_ptr(),
                                   r.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"G": G, "u": u, "x": xn, "r": r, "sums": sums}


def certificate_step(x: torch.Tensor, mu: float, G: Optional[torch.Tensor] = None, form: int = 0,
                     A: Optional[torch.Tensor] = None, Z: Optional[torch.Tensor] = None,
                     m: int = 1) -> Dict[str, torch.Tensor]:
    """The certificate's row terms in one launch (glx_certificate_step; DESIGN.md "Certificate"). form
    0: a row kernel on the given G (with ``m`` the rows of A: on the panel layout a certificate's
    unfused arm takes at (m, n, l), bit-identical to form 1; m = 1: the generic row layout, any n,
    l <= 128); form 1: the epilogue of G = A^T Z (G is computed and returned). Returns {"G", "sums",
    "row_norms"} with sums = [sum_i ||x_i||, max_i ||g_i||, max_i kkt_i, sum_i kkt_i^2, nonzero rows]
    and row_norms = ||g_i|| (both float64)."""
    n, l = x.shape
    dt = _dt(x)
    dev = x.device
    if form == 1:
        if A is None or Z is None:
            raise ValueError("form 1 needs A and Z")
        m = A.shape[0]
        G = torch.full((n, l), float("nan"), dtype=x.dtype, device=dev)
    else:
        if G is None:
            raise ValueError("form 0 needs G")
    sums = _nan_sums(6, dev)
    rn = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    nb = ctypes.c_size_t(0)
    check(lib().glx_certificate_workspace_bytes(dt, m, n, l, ctypes.byref(nb)))
    ws = torch.empty(int(nb.value), dtype=torch.uint8, device=dev)
    check(lib().glx_certificate_step(dt, m, n, l, _ptr(A), _ptr(Z), G.data_ptr(), x.data_ptr(), float(mu),
                                     int(form), rn.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _stream(dev)))
    return {"G": G, "sums": sums[:5], "row_norms": rn}


def admm_primal_step(prod: torch.Tensor, x: torch.Tensor, y: torch.Tensor, z: torch.Tensor,
                     ATb: torch.Tensor, rho: float, tau: float, eta: float, mu: float, thres: float = 1e-3,
                     form: int = 1, w: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The primal ADMM row step (gl_ADMM_primal.py:78-84, glx_admm_primal_step) in one launch.
    ``prod`` is (n, l), or (S, n, l) slabs summed in slab order: Kn w (form 1, direct) or
    g = A^T K (A w) (form 2, Woodbury, which also reads ``w``). With y+ = prod or (w - prod) / rho:
    p = x - (eta rho)((x - y+) - z / rho), x+ = (p max(||p_i|| - eta mu, 0)) / ((||p_i|| < thres) +
    ||p_i||), z+ = z - (tau rho)(x+ - y+), r = x+ - y+, s = y+ - y, w+ = (ATb - z+) + rho x+.
    Returns {"x", "y", "z", "r", "s", "w", "sums"} with sums = [sum_i ||x+_i||, max |x+|] (float64)."""
    n, l = x.shape
    dt = _dt(x)
    dev = x.device
    prod = prod.contiguous()
    S = 1 if prod.dim() == 2 else prod.shape[0]
    if prod.numel() != S * n * l:
        raise ValueError("prod must be (n, l) or (S, n, l)")
    if form == 2 and w is None:
        raise ValueError("form 2 reads w")
    outs = {k: torch.full_like(x, float("nan")) for k in ("x", "y", "z", "r", "s", "w")}
    sums = _nan_sums(2, dev)
    ws = _ws(dt, 1, n, l, dev)
    check(lib().glx_admm_primal_step(dt, n, l, int(form), int(S), prod.data_ptr(), x.data_ptr(), y.data_ptr(),
                                     z.data_ptr(), _ptr(w), ATb.data_ptr(), float(rho), float(tau),
                                     float(eta), float(mu), float(thres), outs["x"].data_ptr(),
                                     outs["y"].data_ptr(), outs["z"].data_ptr(), outs["r"].data_ptr(),
                                     outs["s"].data_ptr(), outs["w"].data_ptr(), sums.data_ptr(),
                                     ws.data_ptr(), ws.numel(), _stream(dev)))
    outs["sums"] = sums
    return outs


def _alm_inner_ws(dtype: int, n: int, l: int, device) -> torch.Tensor:
    nb = ctypes.c_size_t(0)
    check(lib().glx_alm_inner_workspace_bytes(dtype, n, l, ctypes.byref(nb)))
    return torch.empty(int(nb.value), dtype=torch.uint8, device=device)


def alm_inner_step(y: torch.Tensor, u: torch.Tensor, J: torch.Tensor, gamma: float, gamma_next: float,
                   t: float, mu: float, P: Optional[torch.Tensor] = None, Qn: Optional[torch.Tensor] = None,
                   form: int = 0, y_out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """One step of dual ALM's inner loop (gl_ALM_dual.py:56-61, glx_alm_inner_step): with P = Qn y,
    w = y - t (P + J), u+ = (mu w) / max(||w_i||, mu), v = u + (u+ - u) / gamma,
    y+ = (1 - gamma_next) u+ + gamma_next v. form 0: the row kernel on the given ``P``, (n, l) or
    (S, n, l) slabs summed in slab order (the panel layout where the plan of (n, n, l) fuses, the
    generic one elsewhere); form 1: the epilogue of Qn^T y (``Qn`` given). gamma_next = 0: y+ is not
    written (``y_out``, NaN-filled unless passed in, stays as it was). float64 only.
    Returns {"u", "y"}."""
    n, l = y.shape
    dt = _dt(y)
    dev = y.device
    S = 1
    if form == 0:
        if P is None:
            raise ValueError("form 0 needs P")
        P = P.contiguous()
        S = _slabs(P, n, l)
    elif Qn is None:
        raise ValueError("form 1 needs Qn")
    un = torch.full_like(y, float("nan"))
    yn = torch.full_like(y, float("nan")) if y_out is None else y_out
    ws = _alm_inner_ws(dt, n, l, dev)
    check(lib().glx_alm_inner_step(dt, n, l, _ptr(Qn), _ptr(P), int(S), y.data_ptr(), u.data_ptr(), J.data_ptr(),
                                   float(gamma), float(gamma_next), float(t), float(mu), int(form),
                                   un.data_ptr(), yn.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"u": un, "y": yn}


def alm_inner_run(Qn: torch.Tensor, J: torch.Tensor, iters: int, t: float, mu: float,
                  fused: int = 0) -> torch.Tensor:
    """The dual ALM driver's inner loop (glx_alm_inner_run): ``iters`` steps from u = y = 0 with
    gamma = 2 / (i + 1), enqueued back to back; fused: 0 auto, 1 on, 2 off. Returns u."""
    n, l = J.shape
    dt = _dt(J)
    dev = J.device
    u = torch.full_like(J, float("nan"))
    ws = _alm_inner_ws(dt, n, l, dev)
    check(lib().glx_alm_inner_run(dt, n, l, Qn.data_ptr(), J.data_ptr(), int(iters), float(t), float(mu),
                                  int(fused), u.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return u


def _flat_slabs(P: torch.Tensor, count: int, sources: int = 1) -> int:
    """S of a contiguous tensor of sources * S slabs of ``count`` values each."""
    if not P.is_contiguous() or P.numel() % (sources * count) != 0 or P.numel() == 0:
        raise ValueError("slabs must be contiguous, %d x S x %d values" % (sources, count))
    return P.numel() // (sources * count)


def admm_rhs(Ax: torch.Tensor, Au: torch.Tensor, b: torch.Tensor, rho: float) -> torch.Tensor:
    """v = (Ax - rho Au) - b in one launch (glx_admm_rhs, k_admm_v). ``Au`` may be ``Ax`` itself."""
    v = torch.full_like(b, float("nan"))
    check(lib().glx_admm_rhs(_dt(b), b.numel(), Ax.data_ptr(), Au.data_ptr(), b.data_ptr(), float(rho),
                             v.data_ptr(), _stream(b.device)))
    return v


def admm_fin(P: torch.Tensor, b: torch.Tensor, Au: torch.Tensor, s: "Optional[torch.Tensor] | bool" = True
             ) -> Dict[str, Optional[torch.Tensor]]:
    """The dual ADMM finalize in one launch (glx_admm_fin, k_admm_fin). ``P`` holds 2 S slabs of
    b.numel() values, the first source's S then the second's; ``Au`` is the previous A u (read, not
    modified: the kernel works on a copy). ``s``: True allocates it (NaN-filled), None / False passes
    NULL, a tensor is written in place. Returns {"Ax", "Au", "s", "sums"} with
    sums = [sum (Ax - b)^2] (float64)."""
    ml = b.numel()
    S = _flat_slabs(P, ml, 2)
    dev = b.device
    Ax = torch.full_like(b, float("nan"))
    Au_io = Au.clone()
    if s is True:
        s = torch.full_like(b, float("nan"))
    elif s is False:
        s = None
    sums = _nan_sums(1, dev)
    ws = _ws(_dt(b), 1, 1, 1, dev)
    check(lib().glx_admm_fin(_dt(b), ml, S, P.data_ptr(), b.data_ptr(), Ax.data_ptr(), Au_io.data_ptr(), _ptr(s),
                             sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"Ax": Ax, "Au": Au_io, "s": s, "sums": sums}


def admm_primal_rhs(ATb: torch.Tensor, x: torch.Tensor, z: torch.Tensor, rho: float) -> torch.Tensor:
    """w = (ATb - z) + rho x in one launch (glx_admm_primal_rhs, k_admm_primal_w)."""
    w = torch.full_like(x, float("nan"))
    check(lib().glx_admm_primal_rhs(_dt(x), x.numel(), ATb.data_ptr(), x.data_ptr(), z.data_ptr(), float(rho),
                                    w.data_ptr(), _stream(x.device)))
    return w


def admm_primal_fin(P: torch.Tensor, b: torch.Tensor, rho: float, AATb: Optional[torch.Tensor] = None,
                    Az: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None
                    ) -> Dict[str, Optional[torch.Tensor]]:
    """The primal ADMM finalize in one launch (glx_admm_primal_fin, k_admm_primal_fin). ``P`` holds
    S slabs of b.numel() values (direct: ``AATb`` None) or 2 S (Woodbury: ``AATb`` given, the slabs
    of A x then those of A z). ``Az`` and ``v`` are NaN-filled unless passed in; without AATb the
    kernel leaves them as they are. Returns {"Ax", "Az", "v", "sums"}, sums = [sum (Ax - b)^2]."""
    ml = b.numel()
    S = _flat_slabs(P, ml, 2 if AATb is not None else 1)
    dev = b.device
    Ax = torch.full_like(b, float("nan"))
    Az = torch.full_like(b, float("nan")) if Az is None else Az
    v = torch.full_like(b, float("nan")) if v is None else v
    sums = _nan_sums(1, dev)
    ws = _ws(_dt(b), 1, 1, 1, dev)
    check(lib().glx_admm_primal_fin(_dt(b), ml, S, P.data_ptr(), b.data_ptr(), _ptr(AATb), float(rho),
                                    Ax.data_ptr(), Az.data_ptr(), v.data_ptr(), sums.data_ptr(), ws.data_ptr(),
                                    ws.numel(), _stream(dev)))
    return {"Ax": Ax, "Az": Az, "v": v, "sums": sums}


def alm_j(h: torch.Tensor, x: torch.Tensor, rho: float) -> torch.Tensor:
    """J = rho (h - x / rho) in one launch (glx_alm_j, k_alm_j); ``h`` holds S slabs of x.numel()
    values summed in slab order. float64 only."""
    S = _flat_slabs(h, x.numel())
    J = torch.full_like(x, float("nan"))
    check(lib().glx_alm_j(_dt(x), x.numel(), S, h.data_ptr(), x.data_ptr(), float(rho), J.data_ptr(),
                          _stream(x.device)))
    return J


def alm_x(x: torch.Tensor, u: torch.Tensor, g: torch.Tensor, taurho: float, in_place: bool = False,
          x_out: Optional[torch.Tensor] = None, r_out: Optional[torch.Tensor] = None
          ) -> Dict[str, torch.Tensor]:
    """The dual ALM x update in one launch (glx_alm_x, k_alm_x): r = u + g, x+ = x - taurho r with
    ``g`` S slabs of (n, l) summed in slab order. in_place: x+ overwrites a copy of ``x`` handed to
    the kernel as both x and x_out (the solver's call). Returns {"x", "r", "sums"} with
    sums = [sum_i ||x+_i||, max |x+|] (float64). float64 only, l <= 32."""
    n, l = x.shape
    S = _flat_slabs(g, n * l)
    dev = x.device
    if in_place:
        x = x.clone()
        xn = x
    else:
        xn = torch.full_like(x, float("nan")) if x_out is None else x_out
    r = torch.full_like(x, float("nan")) if r_out is None else r_out
    sums = _nan_sums(2, dev)
    ws = _ws(_dt(x), 1, 1, 1, dev)
    check(lib().glx_alm_x(_dt(x), n, l, S, x.data_ptr(), u.data_ptr(), g.data_ptr(), float(taurho),
                          xn.data_ptr(), r.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"x": xn, "r": r, "sums": sums}


def gram(R: torch.Tensor) -> torch.Tensor:
    """R^T R (l x l, float64) accumulated in double over fixed row slabs (glx_gram)."""
    rows, l = R.shape
    out = torch.full((l, l), float("nan"), dtype=torch.float64, device=R.device)
    ws = torch.empty(8 * 256 * l * l, dtype=torch.uint8, device=R.device)
    check(lib().glx_gram(_dt(R), rows, l, R.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                         _stream(R.device)))
    return out


def sym_lambda_max(G) -> float:
    """Largest eigenvalue of a symmetric l x l matrix (l <= 32) by the library's host Jacobi sweep
    (glx_sym_lambda_max); needs no device."""
    import numpy as np
    g = np.ascontiguousarray(np.asarray(G, dtype=np.float64))
    out = ctypes.c_double(0.0)
    check(lib().glx_sym_lambda_max(g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(g.shape[0]),
                                   ctypes.byref(out)))
    return float(out.value)


def _screen_ws(m: int, n: int, device) -> torch.Tensor:
    nb = ctypes.c_size_t(0)
    check(lib().glx_screen_workspace_bytes(int(m), int(n), ctypes.byref(nb)))
    return torch.empty(int(nb.value), dtype=torch.uint8, device=device)


def col_norms(A: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """||a_i||_2 of every column of A in one pass (glx_col_norms): float64, accumulated in double over
    fixed row slabs in slab order. Returns (norms (n,), stats = [max_i ||a_i||, sum_i ||a_i||^2]),
    both float64 device tensors."""
    m, n = A.shape
    dev = A.device
    norms = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    stats = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    ws = _screen_ws(m, n, dev)
    check(lib().glx_col_norms(_dt(A), m, n, A.data_ptr(), norms.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                              ws.numel(), _stream(dev)))
    return norms, stats


def col_norms_sw(A: torch.Tensor, sample_weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The weighted column norms sqrt(sum_j w_j A_ji^2) (glx_col_norms_sw): :func:`col_norms`' slabs and
    combine with one weight per row of A (``sample_weight``: m values of A's dtype on A's device). Returns
    (norms (n,), stats = [max, sum of squares]), float64 device tensors."""
    m, n = A.shape
    dev = A.device
    assert sample_weight.dtype == A.dtype and sample_weight.shape == (m,) and sample_weight.is_contiguous()
    norms = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    stats = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    ws = _screen_ws(m, n, dev)
    check(lib().glx_col_norms_sw(_dt(A), m, n, A.data_ptr(), sample_weight.data_ptr(), norms.data_ptr(),
                                 stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return norms, stats


def cert_fin_sw(P: Optional[torch.Tensor], b: torch.Tensor, sample_weight: Optional[torch.Tensor],
                holdout_weight: Optional[torch.Tensor] = None, want_r: bool = True) -> Dict[str, torch.Tensor]:
    """The weighted residual finalize, one launch (glx_cert_fin_sw). ``P``: (S, m, l) slabs of A x, or
    None for the null product; ``b`` (m, l); the weights m values of b's dtype. Returns {"r": fl(sum of
    the slabs) - b (None without ``want_r``), "rw": fl(w r), "sums": float64 [sum w r^2, sum w r b,
    sum v r^2 (NaN without hold-out weights)]}. ``sample_weight=None`` runs the unweighted finalize
    (k_cert_fin) instead: "rw" is then r itself and "sums" its two values."""
    m, l = b.shape
    dev = b.device
    S = 0 if P is None else int(P.shape[0])
    if P is not None:
        assert P.shape == (S, m, l) and P.is_contiguous() and P.dtype == b.dtype
    for v in (sample_weight, holdout_weight):
        assert v is None or (v.dtype == b.dtype and v.shape == (m,) and v.is_contiguous())
    r = torch.full((m, l), float("nan"), dtype=b.dtype, device=dev) if want_r and sample_weight is not None else None
    rw = torch.full((m, l), float("nan"), dtype=b.dtype, device=dev)
    sums = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    ws = _screen_ws(1, 1, dev)
    check(lib().glx_cert_fin_sw(_dt(b), m, l, None if P is None else P.data_ptr(), S, b.data_ptr(),
                                None if sample_weight is None else sample_weight.data_ptr(),
                                None if holdout_weight is None else holdout_weight.data_ptr(),
                                None if r is None else r.data_ptr(), rw.data_ptr(), sums.data_ptr(), ws.data_ptr(),
                                ws.numel(), _stream(dev)))
    return {"r": r, "rw": rw, "sums": sums}


def screen_step(row_norms: torch.Tensor, col_norms: torch.Tensor, s: float, rho: float,
                mu: float) -> Dict[str, torch.Tensor]:
    """The gap-safe test on n rows (glx_screen_step): row i is kept unless
    s row_norms[i] + col_norms[i] rho < mu holds strictly (a NaN keeps it). Returns {"mask" (n,) uint8,
    "list": int32, n rounded up to 64 entries: the kept rows ascending, then -1 up to count[1] (entries
    past count[1] are left at -2), "count": int32 [kept, kept rounded up to 64]}."""
    n = row_norms.shape[0]
    dev = row_norms.device
    assert row_norms.dtype == torch.float64 and col_norms.dtype == torch.float64
    mask = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    lst = torch.full(((n + 63) // 64 * 64,), -2, dtype=torch.int32, device=dev)
    cnt = torch.full((2,), -2, dtype=torch.int32, device=dev)
    ws = _screen_ws(1, n, dev)
    check(lib().glx_screen_step(n, row_norms.data_ptr(), col_norms.data_ptr(), float(s), float(rho), float(mu),
                                mask.data_ptr(), lst.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(),
                                _stream(dev)))
    return {"mask": mask, "list": lst, "count": cnt}


def gather_cols(src: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dst[r, j] = src[r, idx[j]], 0 where idx[j] is outside src's columns (glx_gather_cols). ``idx``:
    int32, a multiple of 64 entries (the list of :func:`screen_step` up to count[1]). ``out``: a
    contiguous (m, len(idx)) tensor to write (tests put canaries behind it)."""
    m, sw = src.shape
    wp = int(idx.shape[0])
    assert idx.dtype == torch.int32
    dst = torch.full((m, wp), float("nan"), dtype=src.dtype, device=src.device) if out is None else out
    check(lib().glx_gather_cols(_dt(src), m, sw, src.data_ptr(), idx.data_ptr(), wp, dst.data_ptr(),
                                _stream(src.device)))
    return dst


def screen_guard(rec, mu: float, dtype: int, m: int, n: int, l: int, col_max: float, col_sumsq: float,
                 b_norm: float) -> Tuple[float, float, float]:
    """The rounding guard of the screening test (glx_screen_guard, host only, needs no device): from
    the certificate's record to (s_safe, gap+, rho+)."""
    r = (ctypes.c_double * 8)(*[float(v) for v in rec])
    out = (ctypes.c_double * 3)()
    check(lib().glx_screen_guard(r, float(mu), int(dtype), int(m), int(n), int(l), float(col_max),
                                 float(col_sumsq), float(b_norm), out))
    return float(out[0]), float(out[1]), float(out[2])


# ---- feature groups and weights (glx.h "feature groups and weights"; csrc/kernels_group.hip) ----
def _group_args(groups, weights, n: int, l: int = 1):
    """check_groups' host pair (ValueError before any device work), G and the workspace size's G."""
    from .certificate import check_groups
    gw = check_groups(groups if groups is not None else None, weights, n, l)
    if gw is None:
        gw = check_groups(None, [1.0] * int(n), n, l)
    return gw[0], gw[1], int(gw[1].size)


def _group_ws(G: int, device) -> torch.Tensor:
    nb = ctypes.c_size_t(0)
    check(lib().glx_group_workspace_bytes(int(G), ctypes.byref(nb)))
    return torch.empty(int(nb.value), dtype=torch.uint8, device=device)


def group_step(y: torch.Tensor, G: torch.Tensor, xk: torch.Tensor, groups, weights, t: float, mu: float,
               thres: float, theta: float, theta_next: float, out: Optional[Dict[str, torch.Tensor]] = None
               ) -> Dict[str, torch.Tensor]:
    """The grouped FISTA step in one launch (glx_group_step, k_group_fista) on the gradient ``G``:
    (rows, l), or (S, rows, l) slabs summed in slab order. ``groups`` (group_ptr, G + 1 offsets ending
    at n <= rows <= n + 63) and ``weights`` are host arrays; rows from n on belong to no group and come
    back 0. Returns {"xc", "v_next", "y_next", "sums": [sum g (xc - y), sum (xc - y)^2,
    sum_g w_g ||xc_[g]||, max |xc|]}. ``out``: tensors to write instead of fresh ones (tests put
    canaries around them)."""
    rows, l = y.shape
    ptr, w, ng = _group_args(groups, weights, int(groups[-1]) if groups is not None else rows, l)
    n = int(ptr[-1])
    dev = y.device
    S = _slabs(G, rows, l)
    o = out if out is not None else {k: torch.full_like(y, float("nan")) for k in ("xc", "v_next", "y_next")}
    sums = o.get("sums") if out is not None and "sums" in o else _nan_sums(4, dev)
    ws = _group_ws(ng, dev)
    check(lib().glx_group_step(_dt(y), n, rows, l, ng, ptr.ctypes.data, w.ctypes.data, y.data_ptr(), G.data_ptr(),
                               S, xk.data_ptr(), float(t), float(mu), float(thres), float(theta), float(theta_next),
                               o["xc"].data_ptr(), o["v_next"].data_ptr(), o["y_next"].data_ptr(), sums.data_ptr(),
                               ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"xc": o["xc"], "v_next": o["v_next"], "y_next": o["y_next"], "sums": sums}


def group_certificate_step(x: torch.Tensor, G: torch.Tensor, groups, weights, mu: float,
                           want_g: bool = False) -> Dict[str, torch.Tensor]:
    """The certificate's group terms in one launch (glx_group_certificate_step, k_group_cert) on the
    gradient ``G`` ((n, l) or (S, n, l) slabs). Returns {"sums": [sum_g w_g ||x_[g]||,
    max_g ||g_[g]|| / w_g, kkt_max, sum kkt^2, nonzero groups], "group_norms": ||g_[g]|| / w_g
    (G float64)} and, with ``want_g``, "g": the summed gradient."""
    n, l = x.shape
    ptr, w, ng = _group_args(groups, weights, n, l)
    dev = x.device
    S = _slabs(G, n, l)
    sums = _nan_sums(5, dev)
    gn = torch.full((ng,), float("nan"), dtype=torch.float64, device=dev)
    gout = torch.full_like(x, float("nan")) if want_g else None
    ws = _group_ws(ng, dev)
    check(lib().glx_group_certificate_step(_dt(x), n, l, ng, ptr.ctypes.data, w.ctypes.data, x.data_ptr(),
                                           G.data_ptr(), S, float(mu), _ptr(gout), gn.data_ptr(), sums.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _stream(dev)))
    out = {"sums": sums, "group_norms": gn}
    if want_g:
        out["g"] = gout
    return out


def group_cnorm(col_norms: torch.Tensor, groups, weights) -> Tuple[torch.Tensor, torch.Tensor]:
    """gcn[g] = sqrt(sum_{i in [g]} col_norms[i]^2) / w_g in float64 and its maximum (glx_group_cnorm):
    ||A_[g]||_F / w_g from :func:`col_norms`' output. Returns (gcn (G,), max (1,)), device tensors."""
    n = int(col_norms.shape[0])
    assert col_norms.dtype == torch.float64
    ptr, w, ng = _group_args(groups, weights, n)
    dev = col_norms.device
    gcn = torch.full((ng,), float("nan"), dtype=torch.float64, device=dev)
    mx = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    ws = _group_ws(ng, dev)
    check(lib().glx_group_cnorm(n, ng, ptr.ctypes.data, w.ctypes.data, col_norms.data_ptr(), gcn.data_ptr(),
                                mx.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return gcn, mx


def group_expand(kept: torch.Tensor, count: torch.Tensor, group_ptr: torch.Tensor, weights: torch.Tensor,
                 gcn: torch.Tensor, gmap: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Kept groups to kept rows (glx_group_expand, k_group_expand). Device tensors: ``kept`` int32 (the
    list of :func:`screen_step` run on groups), ``count`` int32 (count[0] = K entries of it),
    ``group_ptr`` int32 (G + 1), ``weights`` / ``gcn`` float64 (G), ``gmap`` int32 (G) or None. Returns
    {"rows": int32, n rounded up to 64 entries (the kept rows ascending, -1 up to count[1], -2
    behind), "group_ptr" (G + 1, the first K + 1 written), "weights", "gcn", "map" (G, the first K
    written), "count": int32 [rows, rows rounded up to 64]}; unwritten entries keep -2 / NaN."""
    dev = kept.device
    G = int(weights.shape[0])
    for t in (kept, count, group_ptr) + ((gmap,) if gmap is not None else ()):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert weights.dtype == torch.float64 and gcn.dtype == torch.float64
    assert int(group_ptr.shape[0]) == G + 1 and int(gcn.shape[0]) == G and int(kept.shape[0]) >= 1
    n = int(group_ptr[-1])
    K = int(count[0])
    hk = kept[:K].cpu()
    if not (0 <= K <= G and int(kept.shape[0]) >= K):
        raise ValueError("group_expand: count[0] must be in 0 .. G and within the list")
    if K and not (bool((hk[1:] > hk[:-1]).all()) and int(hk[0]) >= 0 and int(hk[-1]) < G):
        raise ValueError("group_expand: the kept list must be ascending group indices below G")
    rows = torch.full(((n + 63) // 64 * 64,), -2, dtype=torch.int32, device=dev)
    ptr_o = torch.full((G + 1,), -2, dtype=torch.int32, device=dev)
    map_o = torch.full((G,), -2, dtype=torch.int32, device=dev)
    w_o = torch.full((G,), float("nan"), dtype=torch.float64, device=dev)
    gcn_o = torch.full((G,), float("nan"), dtype=torch.float64, device=dev)
    cnt = torch.full((2,), -2, dtype=torch.int32, device=dev)
    check(lib().glx_group_expand(kept.data_ptr(), count.data_ptr(), group_ptr.data_ptr(), weights.data_ptr(),
                                 gcn.data_ptr(), _ptr(gmap), rows.data_ptr(), ptr_o.data_ptr(), w_o.data_ptr(),
                                 gcn_o.data_ptr(), map_o.data_ptr(), cnt.data_ptr(), _stream(dev)))
    return {"rows": rows, "group_ptr": ptr_o, "weights": w_o, "gcn": gcn_o, "map": map_o, "count": cnt}


def group_screen_guard(rec, mu: float, dtype: int, m: int, n: int, l: int, max_run: int, w_min: float,
                       gcol_max: float, col_sumsq: float, b_norm: float) -> Tuple[float, float, float]:
    """The grouped rounding guard (glx_group_screen_guard, host only, needs no device): from the group
    certificate's record to (s_safe, gap+, rho+)."""
    r = (ctypes.c_double * 8)(*[float(v) for v in rec])
    out = (ctypes.c_double * 3)()
    check(lib().glx_group_screen_guard(r, float(mu), int(dtype), int(m), int(n), int(l), int(max_run), float(w_min),
                                       float(gcol_max), float(col_sumsq), float(b_norm), out))
    return float(out[0]), float(out[1]), float(out[2])


# ---- the sparse-group lasso (glx.h "the sparse-group lasso"; csrc/kernels_sgl.hip) ----
def sgl_step(y: torch.Tensor, G: torch.Tensor, xk: torch.Tensor, groups, weights, t: float, mu: float,
             row_ratio: float, thres: float, theta: float, theta_next: float,
             out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """:func:`group_step` with the two-level prox of the sparse-group penalty (glx_sgl_step, k_sgl_fista);
    ``sums[2]`` is row_ratio sum_i ||xc_i|| + (1 - row_ratio) sum_g w_g ||xc_[g]||."""
    rows, l = y.shape
    ptr, w, ng = _group_args(groups, weights, int(groups[-1]) if groups is not None else rows, l)
    n = int(ptr[-1])
    dev = y.device
    S = _slabs(G, rows, l)
    o = out if out is not None else {k: torch.full_like(y, float("nan")) for k in ("xc", "v_next", "y_next")}
    sums = o.get("sums") if out is not None and "sums" in o else _nan_sums(4, dev)
    ws = _group_ws(ng, dev)
    check(lib().glx_sgl_step(_dt(y), n, rows, l, ng, ptr.ctypes.data, w.ctypes.data, y.data_ptr(), G.data_ptr(), S,
                             xk.data_ptr(), float(t), float(mu), float(row_ratio), float(thres), float(theta),
                             float(theta_next), o["xc"].data_ptr(), o["v_next"].data_ptr(), o["y_next"].data_ptr(),
                             sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"xc": o["xc"], "v_next": o["v_next"], "y_next": o["y_next"], "sums": sums}


def sgl_certificate_step(x: torch.Tensor, G: torch.Tensor, groups, weights, mu: float, row_ratio: float,
                         want_g: bool = False) -> Dict[str, torch.Tensor]:
    """The certificate's sparse-group terms in one launch (glx_sgl_certificate_step, k_sgl_cert). Returns
    {"sums": [penalty, max_i ||g_i||, kkt_max, sum kkt^2, nonzero groups, nonzero rows], "row_norms":
    ||g_i|| (n float64)} and, with ``want_g``, "g": the summed gradient."""
    n, l = x.shape
    ptr, w, ng = _group_args(groups, weights, n, l)
    dev = x.device
    S = _slabs(G, n, l)
    sums = _nan_sums(6, dev)
    rn = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    gout = torch.full_like(x, float("nan")) if want_g else None
    ws = _group_ws(ng, dev)
    check(lib().glx_sgl_certificate_step(_dt(x), n, l, ng, ptr.ctypes.data, w.ctypes.data, x.data_ptr(), G.data_ptr(),
                                         S, float(mu), float(row_ratio), _ptr(gout), rn.data_ptr(), sums.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream(dev)))
    out = {"sums": sums, "row_norms": rn}
    if want_g:
        out["g"] = gout
    return out


def sgl_dual_scale(row_norms: torch.Tensor, groups, weights, a: float, cb: float,
                   pads=((1.0, 0.0), (1.0, 0.0))) -> Tuple[torch.Tensor, torch.Tensor]:
    """The per-group dual scalings in one launch (glx_sgl_dual_scale, k_sgl_dual_scale) on the float64 row
    norms: two solves, ``pads[q] = (mul, add)`` applied to every norm first. Returns (s_g (2, G), unclamped;
    min_g s_g (2,)), device tensors."""
    n = int(row_norms.shape[0])
    assert row_norms.dtype == torch.float64 and row_norms.is_contiguous()
    ptr, w, ng = _group_args(groups, weights, n)
    dev = row_norms.device
    sg = torch.full((2, ng), float("nan"), dtype=torch.float64, device=dev)
    neg = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    ws = _group_ws(ng, dev)
    check(lib().glx_sgl_dual_scale(n, ng, ptr.ctypes.data, w.ctypes.data, row_norms.data_ptr(), float(a), float(cb),
                                   float(pads[0][0]), float(pads[0][1]), float(pads[1][0]), float(pads[1][1]),
                                   sg.data_ptr(), neg.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return sg, -neg


def sgl_screen(row_norms: torch.Tensor, col_norms: torch.Tensor, gcn: torch.Tensor, groups, weights, s: float,
               mul: float, add: float, rad: float, a_lo: float, cb_lo: float, group_test: bool = True
               ) -> Dict[str, torch.Tensor]:
    """The two-level screening test in one launch (glx_sgl_screen, k_sgl_screen). Returns {"keep": int32
    (n), "group_keep": int32 (G), "counts": float64 [groups that keep a row, kept rows]}."""
    n = int(row_norms.shape[0])
    for v in (row_norms, col_norms, gcn):
        assert v.dtype == torch.float64 and v.is_contiguous()
    ptr, w, ng = _group_args(groups, weights, n)
    assert int(col_norms.shape[0]) >= n and int(gcn.shape[0]) == ng
    dev = row_norms.device
    keep = torch.full((n,), -2, dtype=torch.int32, device=dev)
    gkeep = torch.full((ng,), -2, dtype=torch.int32, device=dev)
    counts = _nan_sums(2, dev)
    ws = _group_ws(ng, dev)
    check(lib().glx_sgl_screen(n, ng, ptr.ctypes.data, w.ctypes.data, row_norms.data_ptr(), col_norms.data_ptr(),
                               gcn.data_ptr(), float(s), float(mul), float(add), float(rad), float(a_lo),
                               float(cb_lo), int(bool(group_test)), keep.data_ptr(), gkeep.data_ptr(),
                               counts.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"keep": keep, "group_keep": gkeep, "counts": counts}


def sgl_expand(keep: torch.Tensor, group_ptr: torch.Tensor, weights: torch.Tensor, gcn: torch.Tensor,
               gmap: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Kept rows to the reduced problem (glx_sgl_expand, k_sgl_expand). Device tensors: ``keep`` int32 (a
    0/1 flag per row, :func:`sgl_screen`'s), ``group_ptr`` int32 (G + 1), ``weights`` / ``gcn`` float64 (G),
    ``gmap`` int32 (G) or None. Returns {"rows": int32, n rounded up to 64 entries (the kept rows ascending,
    -1 up to count[3], -2 behind), "group_ptr" (G + 1, the first K + 1 written), "weights", "gcn", "map" (G,
    the first K written), "count": int32 [K, rows, rows, rows rounded up to 64]}."""
    dev = keep.device
    G = int(weights.shape[0])
    for t in (keep, group_ptr) + ((gmap,) if gmap is not None else ()):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert weights.dtype == torch.float64 and gcn.dtype == torch.float64
    assert int(group_ptr.shape[0]) == G + 1 and int(gcn.shape[0]) == G
    n = int(group_ptr[-1])
    if int(keep.shape[0]) < n:
        raise ValueError("sgl_expand: keep must hold a flag per row")
    hp = group_ptr.cpu()
    if int(hp[0]) != 0 or not bool((hp[1:] > hp[:-1]).all()):
        raise ValueError("sgl_expand: group_ptr must start at 0 and increase strictly")
    rows = torch.full(((n + 63) // 64 * 64,), -2, dtype=torch.int32, device=dev)
    ptr_o = torch.full((G + 1,), -2, dtype=torch.int32, device=dev)
    map_o = torch.full((G,), -2, dtype=torch.int32, device=dev)
    w_o = torch.full((G,), float("nan"), dtype=torch.float64, device=dev)
    gcn_o = torch.full((G,), float("nan"), dtype=torch.float64, device=dev)
    cnt = torch.full((4,), -2, dtype=torch.int32, device=dev)
    check(lib().glx_sgl_expand(G, keep.data_ptr(), group_ptr.data_ptr(), weights.data_ptr(), gcn.data_ptr(),
                               _ptr(gmap), rows.data_ptr(), ptr_o.data_ptr(), w_o.data_ptr(), gcn_o.data_ptr(),
                               map_o.data_ptr(), cnt.data_ptr(), _stream(dev)))
    return {"rows": rows, "group_ptr": ptr_o, "weights": w_o, "gcn": gcn_o, "map": map_o, "count": cnt}


def sgl_screen_guard(rec, s_pad: float, mu: float, row_ratio: float, dtype: int, m: int, n: int, l: int,
                     max_run: int, w_min: float, col_max: float, col_sumsq: float, b_norm: float,
                     weighted: bool = False) -> Tuple[float, float, float, float, float]:
    """The sparse-group rounding guard (glx_sgl_screen_guard[_sw], host only, needs no device): (mul, add,
    s_safe, gap+, rho+) from the record's first three entries and the padded solve's minimum."""
    r = (ctypes.c_double * 8)(*[float(v) for v in list(rec)[:8]])
    out = (ctypes.c_double * 5)()
    fn = lib().glx_sgl_screen_guard_sw if weighted else lib().glx_sgl_screen_guard
    check(fn(r, float(s_pad), float(mu), float(row_ratio), int(dtype), int(m), int(n), int(l), int(max_run),
             float(w_min), float(col_max), float(col_sumsq), float(b_norm), out))
    return tuple(float(v) for v in out)


# ---- sample weights (glx.h "sample weights"; the weighted guards, host only) ----
def screen_guard_sw(rec, mu: float, dtype: int, m: int, n: int, l: int, col_max: float, col_sumsq: float,
                    b_norm: float) -> Tuple[float, float, float]:
    """The rounding guard of the sample-weighted problem (glx_screen_guard_sw, host only): ``rec`` is
    the weighted certificate's record, the column figures are :func:`col_norms_sw`'s and ``b_norm`` is
    sqrt(sum w b^2)."""
    r = (ctypes.c_double * 8)(*[float(v) for v in rec])
    out = (ctypes.c_double * 3)()
    check(lib().glx_screen_guard_sw(r, float(mu), int(dtype), int(m), int(n), int(l), float(col_max),
                                    float(col_sumsq), float(b_norm), out))
    return float(out[0]), float(out[1]), float(out[2])


def group_screen_guard_sw(rec, mu: float, dtype: int, m: int, n: int, l: int, max_run: int, w_min: float,
                          gcol_max: float, col_sumsq: float, b_norm: float) -> Tuple[float, float, float]:
    """The grouped guard of the sample-weighted problem (glx_group_screen_guard_sw, host only)."""
    r = (ctypes.c_double * 8)(*[float(v) for v in rec])
    out = (ctypes.c_double * 3)()
    check(lib().glx_group_screen_guard_sw(r, float(mu), int(dtype), int(m), int(n), int(l), int(max_run),
                                          float(w_min), float(gcol_max), float(col_sumsq), float(b_norm), out))
    return float(out[0]), float(out[1]), float(out[2])


# ---- an unpenalised intercept (glx.h "an unpenalised intercept"; DESIGN.md "Intercept") ----
def _ic_ws(m: int, n: int, device) -> torch.Tensor:
    nb = ctypes.c_size_t(0)
    check(lib().glx_intercept_workspace_bytes(int(m), int(n), ctypes.byref(nb)))
    return torch.empty(int(nb.value), dtype=torch.uint8, device=device)


def weight_sum(sample_weight, m: int) -> float:
    """sigma = sum_j w_j in float64 on the host, from the weights as they are stored (m without weights)."""
    if sample_weight is None:
        return float(m)
    import numpy as np
    w = sample_weight.detach().cpu().numpy() if isinstance(sample_weight, torch.Tensor) else np.asarray(sample_weight)
    return float(np.sum(w, dtype=np.float64))


def col_norms_ic(A: torch.Tensor, sample_weight: Optional[torch.Tensor] = None,
                 sigma: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The centred weighted column norms sqrt(sum_j w_j (A_ji - a-bar_i)^2) with a-bar_i = sum_j w_j A_ji /
    sigma (glx_col_norms_ic: two launches on :func:`col_norms`' slabs; ``sample_weight`` None: unit weights,
    ``sigma`` None: their float64 sum). Returns (norms (n,), means (n,), stats = [max norm, sum norm^2,
    max |mean|, sum mean^2]), float64 device tensors."""
    m, n = A.shape
    dev = A.device
    if sample_weight is not None:
        assert sample_weight.dtype == A.dtype and sample_weight.shape == (m,) and sample_weight.is_contiguous()
    sigma = weight_sum(sample_weight, m) if sigma is None else float(sigma)
    norms = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    means = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    stats = torch.full((4,), float("nan"), dtype=torch.float64, device=dev)
    ws = _ic_ws(m, n, dev)
    check(lib().glx_col_norms_ic(_dt(A), m, n, A.data_ptr(), _ptr(sample_weight), sigma, norms.data_ptr(),
                                 means.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
    return norms, means, stats


def cert_fin_ic(P: Optional[torch.Tensor], b: torch.Tensor, sample_weight: Optional[torch.Tensor] = None,
                holdout_weight: Optional[torch.Tensor] = None, sigma: Optional[float] = None,
                want_rc: bool = True) -> Dict[str, torch.Tensor]:
    """The centring finalize, its two launches (glx_cert_fin_ic: k_cert_csum, k_cert_fin_c). ``P``: (S, m, l)
    slabs of A x, or None for the null product; ``b`` (m, l); the weights m values of b's dtype or None
    (unit weights). Returns {"rhat": fl(sum of the slabs) - b, "means": its l weighted column means
    (float64), "rc": (T)((double)rhat - mean) (None without ``want_rc``), "rw": fl(w rc), "sums": float64
    [sum w rc^2, sum w rc b, sum v rc^2 (NaN without hold-out weights)]}."""
    m, l = b.shape
    dev = b.device
    S = 0 if P is None else int(P.shape[0])
    if P is not None:
        assert P.shape == (S, m, l) and P.is_contiguous() and P.dtype == b.dtype
    for v in (sample_weight, holdout_weight):
        assert v is None or (v.dtype == b.dtype and v.shape == (m,) and v.is_contiguous())
    sigma = weight_sum(sample_weight, m) if sigma is None else float(sigma)
    rhat = torch.full((m, l), float("nan"), dtype=b.dtype, device=dev)
    rc = torch.full((m, l), float("nan"), dtype=b.dtype, device=dev) if want_rc else None
    rw = torch.full((m, l), float("nan"), dtype=b.dtype, device=dev)
    means = torch.full((l,), float("nan"), dtype=torch.float64, device=dev)
    sums = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    ws = _ic_ws(1, 1, dev)
    check(lib().glx_cert_fin_ic(_dt(b), m, l, _ptr(P), S, b.data_ptr(), _ptr(sample_weight), _ptr(holdout_weight),
                                sigma, rhat.data_ptr(), means.data_ptr(), _ptr(rc), rw.data_ptr(), sums.data_ptr(),
                                ws.data_ptr(), ws.numel(), _stream(dev)))
    return {"rhat": rhat, "means": means, "rc": rc, "rw": rw, "sums": sums}


def screen_guard_ic(rec, mu: float, dtype: int, m: int, n: int, l: int, col_stats, b_norm: float, sigma: float,
                    mean_sq: float) -> Tuple[float, float, float, float]:
    """The rounding guard of the problem with an intercept (glx_screen_guard_ic, host only): ``rec`` the
    centred record, ``col_stats`` :func:`col_norms_ic`'s four values, ``b_norm`` = sqrt(sum w b^2),
    ``mean_sq`` = the sum of the squares of the record's intercept. Returns (s_safe, gap+, rho+, slack)."""
    r = (ctypes.c_double * 8)(*[float(v) for v in rec])
    cs = (ctypes.c_double * 4)(*[float(v) for v in col_stats])
    out = (ctypes.c_double * 4)()
    check(lib().glx_screen_guard_ic(r, float(mu), int(dtype), int(m), int(n), int(l), cs, float(b_norm),
                                    float(sigma), float(mean_sq), out))
    return tuple(float(v) for v in out)


def group_screen_guard_ic(rec, mu: float, dtype: int, m: int, n: int, l: int, max_run: int, w_min: float,
                          gcol_max: float, col_stats, b_norm: float, sigma: float,
                          mean_sq: float) -> Tuple[float, float, float, float]:
    """The grouped guard of the problem with an intercept (glx_group_screen_guard_ic, host only)."""
    r = (ctypes.c_double * 8)(*[float(v) for v in rec])
    cs = (ctypes.c_double * 4)(*[float(v) for v in col_stats])
    out = (ctypes.c_double * 4)()
    check(lib().glx_group_screen_guard_ic(r, float(mu), int(dtype), int(m), int(n), int(l), int(max_run),
                                          float(w_min), float(gcol_max), cs, float(b_norm), float(sigma),
                                          float(mean_sq), out))
    return tuple(float(v) for v in out)
