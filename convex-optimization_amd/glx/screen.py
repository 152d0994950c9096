"""A certified solve of the group-lasso problem with gap-safe screening, and a path over mu.

``solve_certified`` runs libglx's ``glx_certified_solve`` (``csrc/screen.cpp``): FISTA with the exact
group prox and the fixed step 1 / lambda_max(A^T A), stopped when the duality gap of
:func:`glx.certificate` is at most ``tol`` of the primal objective. With ``screen=True`` the
certificate's dual point and gap give, every ``check_every`` iterations, the gap-safe test

    s ||g_i||_2 + ||a_i||_2 sqrt(2 gap) < mu   =>   x*_i = 0        (a_i = column i of A),

under a rounding guard (``glx_screen_guard``); the columns of the rows it proves zero leave A, so the
two passes over A of every later iteration stream a narrower matrix (DESIGN.md "Certified solve and
screening"). ``path`` solves a decreasing sequence of mu, each warm-started from the one before,
with the column norms and lambda_max computed once. Everything runs on the GPU; there is no CPU path.

With ``groups`` / ``weights`` (:mod:`glx.certificate`: contiguous row ranges as a ``group_ptr`` array,
weights w_g > 0) the penalty is ``mu sum_g w_g ||x_[g]||_F``, the step is the plain A^T r followed by
the group kernel, and the test runs on groups,

    s ||g_[g]||_F / w_g + (||A_[g]||_F / w_g) sqrt(2 gap) < mu   =>   x*_[g] = 0,

so that proving a group zero removes all its columns from A at once (``glx_group_certified_solve``;
DESIGN.md "Feature groups and weights").

With ``fit_intercept=True`` the loss carries an unpenalised intercept, ``1/2 sum_j w_j ||(A x + 1 c^T -
b)_j||^2``, which is eliminated exactly: the residual is centred between the two dense passes, the step
is 1 / lambda_max(A^T W P A) and the test uses the centred column norms (the ``_ic`` entries; DESIGN.md
"Intercept"). A is never centred or copied.
"""
from __future__ import annotations

import ctypes
import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import GlxCertifiedInfo, GlxGroupCertifiedInfo, GlxProblem, GlxSglCertifiedInfo, check, lib
from .certificate import (_inputs, _np_dtype, _rows_of, _sigma, _sw_device, check_groups, check_row_ratio,
                          check_sample_weight, compose, compose_groups, mu_max)

DEFAULT_MAXIT = 100000


def mu_grid(mu_top: float, n_mus: int = 10, mu_min_ratio: float = 1e-2) -> List[float]:
    """The decreasing geometric grid of ``n_mus`` values from ``mu_top`` down to
    ``mu_min_ratio * mu_top`` (a single value: ``mu_top``). Host only."""
    mu_top = float(mu_top)
    n_mus = int(n_mus)
    if not (mu_top > 0.0 and math.isfinite(mu_top)):
        raise ValueError("mu_max must be positive and finite (is A^T b zero?)")
    if n_mus < 1:
        raise ValueError("n_mus must be >= 1")
    if not 0.0 < float(mu_min_ratio) < 1.0:
        raise ValueError("mu_min_ratio must be in (0, 1)")
    if n_mus == 1:
        return [mu_top]
    q = float(mu_min_ratio) ** (1.0 / (n_mus - 1))
    return [mu_top * q ** i for i in range(n_mus)]


def _check_mus(mus: Sequence[float]) -> List[float]:
    out = [float(v) for v in mus]
    if not out:
        raise ValueError("mus is empty")
    if any(not (v >= 0.0 and math.isfinite(v)) for v in out):
        raise ValueError("every mu must be >= 0 and finite")
    if any(b >= a for a, b in zip(out, out[1:])):
        raise ValueError("mus must be strictly decreasing (each solve warm-starts the next)")
    return out


def _check_args(A, b, x0, tol, maxit, check_every, groups=None, weights=None):
    """The argument checks that need no device (shapes from the arrays as they are). Returns
    :func:`glx.certificate.check_groups`' pair, None for the row problem."""
    sa, sb = tuple(np.shape(A)), tuple(np.shape(b))
    if len(sa) != 2 or len(sb) != 2:
        raise ValueError("A and b must be 2-D (group lasso with l columns)")
    if sa[0] != sb[0]:
        raise ValueError("shape mismatch: A %s, b %s" % (sa, sb))
    if x0 is not None and tuple(np.shape(x0)) != (sa[1], sb[1]):
        raise ValueError("shape mismatch: A %s, b %s, x0 %s" % (sa, sb, tuple(np.shape(x0))))
    if not float(tol) > 0.0:
        raise ValueError("tol must be positive")
    if int(maxit) < 0:
        raise ValueError("maxit must be >= 0")
    if int(check_every) < 1:
        raise ValueError("check_every must be >= 1")
    return check_groups(groups, weights, sa[1], sb[1])


def _check_sample(A, sample_weight, holdout_weight):
    """The host checks of the two observation-weight vectors (glx.certificate.check_sample_weight),
    before any device work: ``(sw, hw)`` in A's dtype, None where not given. Hold-out weights without
    sample weights are held out of the unweighted fit: sw = ones."""
    m, dt = _rows_of(A), _np_dtype(A)
    sw = check_sample_weight(sample_weight, m, dt)
    hw = check_sample_weight(holdout_weight, m, dt, "holdout_weight")
    if hw is not None and sw is None:
        sw = np.ones(m, dtype=dt)
    return sw, hw


def _describe(fn, *args) -> str:
    """The line of one of libglx's host-only ``*_describe`` entries."""
    buf = ctypes.create_string_buffer(2048)
    check(fn(*args, buf, len(buf)))
    return buf.value.decode()


def _holdout_info(info: Dict[str, Any], hw) -> None:
    """holdout_loss = 1/2 sum_j v_j ||(A x - b)_j||^2 / sum_j v_j from the solve's holdout_sum."""
    if hw is not None:
        info["holdout_loss"] = 0.5 * info["holdout_sum"] / float(np.sum(hw, dtype=np.float64))


class _Prepared:
    """What a sequence of solves on one (A, b) shares: the device copies, the step, the column norms
    and the workspace."""

    def __init__(self, A, b, screen: bool, comm=None, gw=None, sw=None, weighted: bool = False,
                 intercept: bool = False, tau: float = 0.0):
        """``sw``: the checked host sample weights (None: the unweighted problem). ``weighted=True``
        sizes the workspace for weights that arrive later (:meth:`set_weights`, one per fold).
        ``intercept=True``: the problem with an unpenalised intercept (libglx's ``_ic`` entries, which
        take the weights or none). ``tau`` > 0: the sparse-group penalty (the checked ``row_ratio``; libglx's
        ``glx_sgl`` entries, which take the weights or none)."""
        self.tau = float(tau)
        if comm is not None:
            raise ValueError("the certified solve is single-GPU: it takes no communicator")
        _, self.Ad, self.bd = _inputs(None, A, b)
        self.numpy = not isinstance(A, torch.Tensor)
        self.m, self.n = self.Ad.shape
        self.l = self.bd.shape[1]
        self.device = self.Ad.device
        self.gdt = _lib.GLX_F64 if self.Ad.dtype == torch.float64 else _lib.GLX_F32
        self.screen = bool(screen)
        self.gw = gw   # (group_ptr, weights) on the host, or None: rows
        self.G = 0 if gw is None else int(gw[1].size)
        self.max_run = 0 if gw is None else int(np.diff(gw[0]).max())
        self.intercept = bool(intercept)
        self.weighted = bool(weighted) or sw is not None or self.intercept
        with torch.cuda.device(self.device):
            nb = ctypes.c_size_t(0)   # (first: it refuses what the solve would, before any launch)
            suffix = "_ic" if self.intercept else ("_sw" if self.weighted else "")
            if self.tau > 0.0:
                check(lib().glx_sgl_certified_workspace_bytes(self.gdt, self.m, self.n, self.l, self.G,
                                                              int(self.screen), int(self.weighted), ctypes.byref(nb)))
            elif gw is None:
                check(getattr(lib(), "glx_certified%s_workspace_bytes" % suffix)(
                    self.gdt, self.m, self.n, self.l, int(self.screen), ctypes.byref(nb)))
            else:
                check(getattr(lib(), "glx_group_certified%s_workspace_bytes" % suffix)(
                    self.gdt, self.m, self.n, self.l, self.G, int(self.screen), ctypes.byref(nb)))
            self.set_weights(sw)
            self.ws = torch.empty(int(nb.value), dtype=torch.uint8, device=self.device)

    def set_weights(self, sw):
        """The figures that depend on the sample weights (host array of A's dtype, or None): the step
        1 / lambda_max(A^T W A) and the (weighted) column norms. A, b and the workspace stay."""
        from . import kernels
        from .solver import _lambda_max
        if sw is not None and not self.weighted:
            raise ValueError("this preparation was sized for the unweighted problem")
        with torch.cuda.device(self.device):
            self.sw = _sw_device(sw, self.device)
            if self.intercept:
                # sigma on the host in float64 from the weights as rounded to A's dtype; the step is
                # 1 / lambda_max(A^T W P A) and the column figures are the centred ones
                self.sigma = _sigma(sw, self.m)
                self.lam = float(_lambda_max(self.Ad, sample_weight=self.sw, center_sum=self.sigma))
                self.t = 1.0 / self.lam
                self.cn = self.cstats = None
                if self.screen:
                    self.cn, _, st = kernels.col_norms_ic(self.Ad, self.sw, self.sigma)
                    self.cstats = (ctypes.c_double * 4)(*st.cpu().tolist())
                return
            self.lam = float(_lambda_max(self.Ad, sample_weight=self.sw))
            self.t = 1.0 / self.lam
            self.cn = self.cstats = None
            if self.screen:
                self.cn, st = (kernels.col_norms(self.Ad) if self.sw is None
                               else kernels.col_norms_sw(self.Ad, self.sw))
                self.cstats = (ctypes.c_double * 2)(*st.cpu().tolist())

    def solve(self, mu: float, x0, tol: float, maxit: int, check_every: int, hold=None):
        """``hold``: hold-out weights (a device tensor of A's dtype, m values) for the final certificate;
        ``info`` then carries ``holdout_sum`` = sum_j hold_j ||(A x - b)_j||^2."""
        mu = float(mu)
        if not mu >= 0.0:
            raise ValueError("mu must be >= 0")
        xd, _, _ = _inputs(x0, self.Ad, self.bd)
        if x0 is not None:
            xd = xd.clone()   # the solve works in place
        p = GlxProblem(dtype=self.gdt, method=0, m=self.m, n=self.n, l=self.l, A=self.Ad.data_ptr(),
                       b=self.bd.data_ptr(), x=xd.data_ptr(), mu0=mu, comm=None)
        rows = torch.full(((self.n + 63) // 64 * 64,), -1, dtype=torch.int32, device=self.device)
        if hold is not None and self.sw is None:
            raise ValueError("hold-out weights go with sample weights")
        if self.gw is not None:
            return self._solve_groups(mu, xd, p, rows, tol, maxit, check_every, hold)
        info = GlxCertifiedInfo()
        hs = ctypes.c_double(0.0)
        icpt = (ctypes.c_double * self.l)()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            cn = None if self.cn is None else self.cn.data_ptr()
            if self.intercept:
                check(lib().glx_certified_solve_ic(ctypes.byref(p), None if self.sw is None else self.sw.data_ptr(),
                                                   None if hold is None else hold.data_ptr(), self.sigma, self.t,
                                                   float(tol), int(maxit), int(self.screen), int(check_every), cn,
                                                   self.cstats, rows.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                   ctypes.byref(info), ctypes.byref(hs), icpt, stream))
            elif self.sw is None:
                check(lib().glx_certified_solve(ctypes.byref(p), self.t, float(tol), int(maxit), int(self.screen),
                                                int(check_every), cn, self.cstats, rows.data_ptr(),
                                                self.ws.data_ptr(), self.ws.numel(), ctypes.byref(info), stream))
            else:
                check(lib().glx_certified_solve_sw(ctypes.byref(p), self.sw.data_ptr(),
                                                   None if hold is None else hold.data_ptr(), self.t, float(tol),
                                                   int(maxit), int(self.screen), int(check_every), cn, self.cstats,
                                                   rows.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                   ctypes.byref(info), ctypes.byref(hs), stream))
        out: Dict[str, Any] = compose(list(info.cert), mu)
        if self.intercept:
            out["plan"] = _describe(lib().glx_certified_ic_describe, self.gdt, self.m, self.n, self.l, int(self.screen))
            out["intercept"] = np.array(list(icpt), dtype=np.float64)
        else:
            out["plan"] = (_lib.certified_describe(self.gdt, self.m, self.n, self.l, self.screen) if self.sw is None
                           else _describe(lib().glx_certified_sw_describe, self.gdt, self.m, self.n, self.l,
                                          int(self.screen)))
        if hold is not None:
            out["holdout_sum"] = float(hs.value)
        nc = int(info.compactions)
        if int(info.listed) > 0:
            kept_rows = rows[:int(info.listed)].cpu().numpy().astype(np.int64)
            kept_rows = kept_rows[kept_rows >= 0]
        elif self.screen and int(info.kept) == 0 and int(info.checks) > 0:
            kept_rows = np.zeros(0, dtype=np.int64)
        else:
            kept_rows = np.arange(self.n, dtype=np.int64)
        out.update(converged=bool(info.converged), iterations=int(info.iters), checks=int(info.checks),
                   compactions=nc, kept_history=[int(info.kept_hist[i]) for i in range(min(nc, 64))],
                   kept=int(info.kept), kept_rows=kept_rows, width=int(info.width), rounds=int(info.rounds),
                   passes=float(info.passes), tt=float(info.tt), inner_rel_gap=float(info.inner_rel_gap),
                   step_fused=bool(info.fused), screen=self.screen, tol=float(tol), step=self.t, mu=mu)
        return xd, out

    def _solve_groups(self, mu, xd, p, rows, tol, maxit, check_every, hold=None):
        ptr, w = self.gw
        sinfo = GlxSglCertifiedInfo()
        ginfo = sinfo.base if self.tau > 0.0 else GlxGroupCertifiedInfo()
        hs = ctypes.c_double(0.0)
        grps = torch.full((self.G,), -1, dtype=torch.int32, device=self.device)
        icpt = (ctypes.c_double * self.l)()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            cn = None if self.cn is None else self.cn.data_ptr()
            if self.tau > 0.0:
                check(lib().glx_sgl_certified_solve_sw(
                    ctypes.byref(p), self.tau, self.G, ptr.ctypes.data, w.ctypes.data,
                    None if self.sw is None else self.sw.data_ptr(), None if hold is None else hold.data_ptr(),
                    self.t, float(tol), int(maxit), int(self.screen), int(check_every), cn, self.cstats,
                    rows.data_ptr(), grps.data_ptr(), self.ws.data_ptr(), self.ws.numel(), ctypes.byref(sinfo),
                    ctypes.byref(hs), stream))
            elif self.intercept:
                check(lib().glx_group_certified_solve_ic(
                    ctypes.byref(p), self.G, ptr.ctypes.data, w.ctypes.data,
                    None if self.sw is None else self.sw.data_ptr(), None if hold is None else hold.data_ptr(),
                    self.sigma, self.t, float(tol), int(maxit), int(self.screen), int(check_every), cn, self.cstats,
                    rows.data_ptr(), grps.data_ptr(), self.ws.data_ptr(), self.ws.numel(), ctypes.byref(ginfo),
                    ctypes.byref(hs), icpt, stream))
            elif self.sw is None:
                check(lib().glx_group_certified_solve(
                    ctypes.byref(p), self.G, ptr.ctypes.data, w.ctypes.data, self.t, float(tol), int(maxit),
                    int(self.screen), int(check_every), cn, self.cstats,
                    rows.data_ptr(), grps.data_ptr(), self.ws.data_ptr(), self.ws.numel(), ctypes.byref(ginfo),
                    stream))
            else:
                check(lib().glx_group_certified_solve_sw(
                    ctypes.byref(p), self.G, ptr.ctypes.data, w.ctypes.data, self.sw.data_ptr(),
                    None if hold is None else hold.data_ptr(), self.t, float(tol), int(maxit), int(self.screen),
                    int(check_every), cn, self.cstats, rows.data_ptr(), grps.data_ptr(), self.ws.data_ptr(),
                    self.ws.numel(), ctypes.byref(ginfo), ctypes.byref(hs), stream))
        info = ginfo.base
        out: Dict[str, Any] = compose_groups(list(info.cert), mu)
        if self.tau > 0.0:   # the sparse-group record: cert[7] counts the nonzero rows
            nzr = float(info.cert[7])
            out["fused"] = False
            out["nonzero_rows"] = nzr if math.isnan(nzr) else int(nzr)
            out["row_ratio"] = self.tau
            out["plan"] = _describe(lib().glx_sgl_certified_describe, self.gdt, self.m, self.n, self.l, self.max_run,
                                    int(self.screen), int(self.sw is not None))
        elif self.intercept:
            out["plan"] = _describe(lib().glx_group_certified_ic_describe, self.gdt, self.m, self.n, self.l,
                                    self.max_run, int(self.screen))
            out["intercept"] = np.array(list(icpt), dtype=np.float64)
        else:
            out["plan"] = (_lib.group_certified_describe(self.gdt, self.m, self.n, self.l, self.max_run, self.screen)
                           if self.sw is None else
                           _describe(lib().glx_group_certified_sw_describe, self.gdt, self.m, self.n, self.l,
                                     self.max_run, int(self.screen)))
        if hold is not None:
            out["holdout_sum"] = float(hs.value)
        nc = int(info.compactions)
        if int(ginfo.listed_groups) > 0:
            kept_groups = grps[:int(ginfo.listed_groups)].cpu().numpy().astype(np.int64)
            kept_rows = rows[:int(info.listed)].cpu().numpy().astype(np.int64)
            kept_rows = kept_rows[kept_rows >= 0]
        elif self.screen and int(info.kept) == 0 and int(info.checks) > 0:
            kept_groups = np.zeros(0, dtype=np.int64)
            kept_rows = np.zeros(0, dtype=np.int64)
        else:
            kept_groups = np.arange(self.G, dtype=np.int64)
            kept_rows = np.arange(self.n, dtype=np.int64)
        out.update(converged=bool(info.converged), iterations=int(info.iters), checks=int(info.checks),
                   compactions=nc, kept_history=[int(info.kept_hist[i]) for i in range(min(nc, 64))],
                   kept=int(info.kept), kept_groups=kept_groups, kept_rows=kept_rows, width=int(info.width),
                   rounds=int(info.rounds), passes=float(info.passes), tt=float(info.tt),
                   inner_rel_gap=float(info.inner_rel_gap), step_fused=False, screen=self.screen, tol=float(tol),
                   step=self.t, mu=mu)
        if self.tau > 0.0:
            out["kept_row_history"] = [int(sinfo.kept_row_hist[i]) for i in range(min(nc, 64))]
        return xd, out

    def result(self, xd: torch.Tensor):
        return xd.cpu().numpy() if self.numpy else xd


def solve_certified(A, b, mu, x0=None, tol: float = 1e-6, maxit: int = DEFAULT_MAXIT, screen: bool = True,
                    check_every: int = 10, comm=None, groups=None, weights=None, sample_weight=None,
                    holdout_weight=None, fit_intercept: bool = False, row_ratio=None) -> Tuple[Any, Dict[str, Any]]:
    """Solve min_x 1/2 ||A x - b||_F^2 + mu sum_i ||x_i||_2 until the duality gap is at most ``tol``
    of the primal objective (or ``maxit`` iterations in total).

    ``A`` (m x n), ``b`` (m x l) and ``x0`` (n x l, default 0) are NumPy arrays or torch tensors and
    are not modified; the computation runs in A's dtype. Returns ``(x, info)``: x as A's kind of
    array, and ``info`` with the keys of :func:`glx.certificate` for the returned x on the full
    problem (``primal``, ``dual``, ``gap``, ``rel_gap``, ``scale``, ``gmax``, ``kkt_max``, ``kkt_fro``,
    ``nonzero_rows``, ``fused``, ``plan``) plus ``converged`` (rel_gap <= tol), ``iterations``,
    ``checks``, ``compactions``, ``kept_history`` (rows kept after each compaction), ``kept`` (rows the last screening test did not
    prove zero), ``kept_rows`` (their indices, ascending: every other row is zero at the optimum, and +0
    in the returned x),
    ``width`` (columns of the last reduced problem), ``rounds``, ``passes`` (passes over A, each
    weighted by its width / n), ``tt`` (seconds inside the native call) and ``step``. Single GPU: a
    communicator is refused.

    ``groups`` / ``weights`` (both None: the row problem, today's path and bits): solve
    ``mu sum_g w_g ||x_[g]||_F`` over contiguous row ranges (``group_ptr`` array; ``weights`` alone:
    single rows). ``info`` then carries ``nonzero_groups`` in place of ``nonzero_rows``, ``kept`` and
    ``kept_history`` count groups, and ``kept_groups`` (ascending) stands next to ``kept_rows`` (the
    rows of those groups).

    ``sample_weight`` (None: today's path, bit for bit): m observation weights ``w_j >= 0``, at least one
    > 0, rounded once to A's dtype: solve ``1/2 sum_j w_j ||(A x - b)_j||^2 + mu Omega(x)`` on the
    caller's A (no copy, no scaling; a 0/1 vector solves the row-subset problem, integer weights the
    row-duplicated one). The step is 1 / lambda_max(A^T W A), screening runs on the weighted column
    norms under the weighted guard, and ``info`` speaks of the weighted problem. ``holdout_weight``
    (m values >= 0): ``info["holdout_loss"]`` = 1/2 sum_j v_j ||(A x - b)_j||^2 / sum_j v_j of the
    returned x, from the final certificate's own launch (``holdout_sum`` is the numerator's sum).

    ``fit_intercept`` (False: today's path, call for call and bit for bit): solve
    ``min_{x, c} 1/2 sum_j w_j ||(A x + 1 c^T - b)_j||^2 + mu Omega(x)`` with an unpenalised intercept c in
    R^l (DESIGN.md "Intercept"). c is eliminated exactly, so the iteration is the same FISTA with the
    residual centred between the two dense passes, the step is 1 / lambda_max(A^T W P A) and screening
    runs on the centred weighted column norms; A is not centred or copied. ``info["intercept"]`` holds c
    (l float64 values), ``primal`` / ``dual`` / ``gap`` / ``rel_gap`` speak of the minimum over c, and
    ``holdout_loss`` = 1/2 sum_j v_j ||(A x + c - b)_j||^2 / sum_j v_j. It composes with ``groups`` /
    ``weights``, ``sample_weight`` and ``holdout_weight``.

    ``row_ratio`` (None or 0: today's group path, call for call and bit for bit; needs ``groups`` /
    ``weights``): tau in [0, 1], the sparse-group lasso ``mu (tau sum_i ||x_i||_2 + (1 - tau) sum_g w_g
    ||x_[g]||_F)`` (DESIGN.md "Sparse-group lasso"): the step is the two-level prox, the test screens groups
    and, inside a surviving group, rows, and a compaction removes both. ``info`` carries the group keys plus
    ``row_ratio``, ``nonzero_rows`` beside ``nonzero_groups`` and ``kept_row_history`` (rows after each
    compaction; ``kept`` and ``kept_history`` keep counting groups). It composes with ``sample_weight`` and
    ``holdout_weight``; with ``fit_intercept=True`` it raises ValueError (the intercept guard's slack has no
    sparse-group derivation yet)."""
    gw = _check_args(A, b, x0, tol, maxit, check_every, groups, weights)
    tau = check_row_ratio(row_ratio, gw, fit_intercept)
    sw, hw = _check_sample(A, sample_weight, holdout_weight)
    if not float(mu) >= 0.0:
        raise ValueError("mu must be >= 0")
    prep = _Prepared(A, b, screen, comm, gw, sw, intercept=bool(fit_intercept), tau=tau)
    xd, info = prep.solve(mu, x0, tol, maxit, check_every, _sw_device(hw, prep.device))
    _holdout_info(info, hw)
    return prep.result(xd), info


def path(A, b, mus: Optional[Sequence[float]] = None, n_mus: int = 10, mu_min_ratio: float = 1e-2,
         **kw) -> List[Tuple[float, Any, Dict[str, Any]]]:
    """Certified solves over a decreasing sequence of mu: ``mus``, or the geometric grid of ``n_mus``
    values from ``glx.mu_max(A, b)`` down to ``mu_min_ratio`` of it (:func:`mu_grid`). Each solve is
    warm-started from the one before; the column norms and lambda_max are computed once. ``kw``:
    ``tol``, ``maxit``, ``screen``, ``check_every``, ``groups``, ``weights``, ``sample_weight``,
    ``holdout_weight``, ``fit_intercept``, ``row_ratio`` of :func:`solve_certified` (with groups, sample
    weights, an intercept or a row ratio the grid starts at their ``mu_max``). Returns the list of ``(mu, x, info)``; at mu = mu_max
    the entry is x = 0 with gap 0 and no iterations (with an intercept the gap there is rounding dust:
    the centred residual sums to zero only up to its own rounding)."""
    unknown = set(kw) - {"tol", "maxit", "screen", "check_every", "comm", "groups", "weights", "sample_weight",
                         "holdout_weight", "fit_intercept", "row_ratio"}
    if unknown:
        raise TypeError("path() got unexpected keyword arguments %s" % sorted(unknown))
    tol, maxit = kw.get("tol", 1e-6), kw.get("maxit", DEFAULT_MAXIT)
    check_every = kw.get("check_every", 10)
    gw = _check_args(A, b, None, tol, maxit, check_every, kw.get("groups"), kw.get("weights"))
    tau = check_row_ratio(kw.get("row_ratio"), gw, bool(kw.get("fit_intercept", False)))
    sw, hw = _check_sample(A, kw.get("sample_weight"), kw.get("holdout_weight"))
    if mus is not None:
        mus = _check_mus(mus)
    else:
        mu_grid(1.0, n_mus, mu_min_ratio)   # the grid's own checks, before any device work
    prep = _Prepared(A, b, kw.get("screen", True), kw.get("comm"), gw, sw,
                     intercept=bool(kw.get("fit_intercept", False)), tau=tau)
    if mus is None:
        mus = mu_grid(_top(prep, gw, sw), n_mus, mu_min_ratio)
    return _run_path(prep, mus, tol, maxit, check_every, hw)


def _top(prep: "_Prepared", gw, sw) -> float:
    if prep.tau > 0.0:
        return mu_max(prep.Ad, prep.bd, gw[0], gw[1], sample_weight=sw, row_ratio=prep.tau)
    if prep.intercept:
        return mu_max(prep.Ad, prep.bd, None if gw is None else gw[0], None if gw is None else gw[1],
                      sample_weight=sw, fit_intercept=True)
    if sw is not None:
        return mu_max(prep.Ad, prep.bd, None if gw is None else gw[0], None if gw is None else gw[1], sample_weight=sw)
    return mu_max(prep.Ad, prep.bd) if gw is None else mu_max(prep.Ad, prep.bd, gw[0], gw[1])


def _run_path(prep: "_Prepared", mus, tol, maxit, check_every, hw=None):
    """The warm-started solves of :func:`path` on a prepared problem (its current weights)."""
    hold = _sw_device(hw, prep.device)
    out = []
    xd = None
    for mu in mus:
        xd, info = prep.solve(mu, xd, tol, maxit, check_every, hold)
        _holdout_info(info, hw)
        out.append((mu, prep.result(xd.clone()), info))
    return out
