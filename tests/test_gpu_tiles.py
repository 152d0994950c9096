"""Every tile of the two dense products, by name, at the shapes where the planner picks it.

A @ X - B (glx_residual, glx_residual_batch) and A^T R (glx_gradient) are called with ctypes on
caller-owned buffers. The table is tile_cases.ROWS (one row per admitted tile, dtype and count of
right-hand sides; test_tiles_cpu.py checks it on the host); every case first asserts that
glx_plan_describe shows the kernel and K split it names, then runs:

(a) Position-coded integers, compared for equality. A[i,k] = ((7i + 3k) mod 5) - 2,
    X_s[k,j] = ((5k + 11j + 3s) mod 3) - 1, B[i,j] = ((3i + 5j) mod 7) - 3 and, for A^T R,
    R[i,j] = ((5i + 3j) mod 7) - 3. With n <= 2046 every product, partial sum, residual and square
    is an integer below 2^24, exact in fp32 and fp64 in any summation order, so R, G,
    h = 0.5 sum r^2 and sq = sum r^2 must equal the int64 reference bit for bit: a dropped or
    repeated chunk, a split boundary, a tail row that takes its neighbour's data or swapped
    sources all show. Tolerance zero.
(b) Random values whose rows are scaled by {1e-3, 1, 30} (A's rows and X's, R's for A^T R),
    compared elementwise with the product in the next wider type (np.longdouble for f64 inputs,
    np.float64 for f32):
        |R - ref| <= (n + 2) eps_T (|A||X| + |B|),     |G - ref| <= (m + 2) eps_T |A|^T |R|,
    the worst case of an n-term dot product summed in any order plus the subtraction, eps = 2u
    covering the second-order terms (the bar test_gpu_admm.py uses for A^T Z). h and sq are held
    against the sum of squares of the R the kernel returned, taken in longdouble, within
    (eps_T + D eps64) sum r^2: the squares round once in T (k_finalize_residual forms
    (double)(r * r)), and the fp64 accumulation (grid_reduce) is at most D = 32 additions deep:
    one element per thread at these sizes, 6 shuffle levels and 2 for the waves in the workgroup,
    then 4 + 6 + 2 over the block partials, 21 in all (the sibling modules use 32 too).
(c) NaN where NumPy puts it, after the clean run of (a). IEEE gives 0 * NaN = NaN and NumPy
    follows it, so an element is NaN exactly where a NaN enters its dot product, whatever the
    other factor (the integer A has zeros: a kernel that skipped them would differ here).
    A[m-1,n-1] = NaN: row m-1 of every R_s, and h / sq. X_1[n-1,l/2] = NaN (X_0 with one
    right-hand side): column l/2 of that R_s and its sq, nothing in the other sources. For A^T R,
    R[m-1,l/2] = NaN: column l/2 of G; A[m-1,n-1] = NaN: row n-1 of G. Every element outside is
    bit-identical to the clean run.
Every launch of (a) and (b) is made twice and must give identical bits.

Guard bands: every buffer is carved from one allocation with 4 KiB on both sides (interior
pointers stay 256-byte aligned). Bands of inputs hold NaN, so an over-read that reaches a result
shows there; bands of outputs (each R_s, G, h, sq) and the band behind the workspace, which is
exactly glx_kernel_workspace_bytes long, hold a fixed byte pattern. After each launch everything
but the outputs' and the workspace's own bytes must be unchanged. The outputs start as that
pattern and the workspace as NaN, so an element nobody wrote shows too.

Measured on an MI355X, worst error / bar over all cases of (b); the module prints this table when
its tests are over (pytest -s):
  A @ X - B   R      f64 0.153   f32 0.109
              h, sq  f64 0.0281  f32 0.174
  A^T R       G      f64 0.286   f32 0.292
None is above 1. (The largest ratios come from the shortest sums: at one chunk or one row step the
bar is a few eps.) All 379 cases pass on the kernels as they are. Against a library built with
four wrong results put in for a trial (the LDS tiles' tail chunk dropped, the DMA ring's last odd
chunk dropped, wave 3 left out of the A^T R panel sum, two sources swapped in the three-source
direct-load kernel) the cases of exactly those kernels failed, 249 of 379.
"""
import ctypes
import functools
import json

import numpy as np
import pytest

import tile_cases

pytestmark = pytest.mark.gpu

BAND = 4096
PATTERN = 0xA5
D_SUM = 32
MEASURED = {}
CASES = tile_cases.cases()


def _note(key, ratio):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nworst error / bar:", json.dumps({k: float("%.3g" % v) for k, v in sorted(MEASURED.items())}))


def _np(dtype):
    return np.float64 if dtype == "f64" else np.float32


def _wide(T):
    return np.longdouble if T == np.float64 else np.float64


# ---------------------------------------------------------------------------------------------
# buffers with guard bands
# ---------------------------------------------------------------------------------------------
class Arena:
    """Host image of one device allocation: [band | buffer, padded to 256 B | band] per buffer."""

    def __init__(self):
        self.parts, self.at, self.size = [], {}, 0

    def _fill(self, nbytes, kind, T):
        if kind == "in":   # NaN of the buffer's type
            return np.full(nbytes // np.dtype(T).itemsize, np.nan, dtype=T).view(np.uint8)
        return np.full(nbytes, PATTERN, dtype=np.uint8)

    def add(self, name, kind, T=np.float64, data=None, nbytes=None):
        """kind: "in" (data given), "out" (nbytes of pattern), "ws" (nbytes of NaN bytes, pattern bands)."""
        if data is not None:
            payload = np.ascontiguousarray(data, dtype=T).view(np.uint8).reshape(-1)
        else:
            payload = np.full(nbytes, 0xFF if kind == "ws" else PATTERN, dtype=np.uint8)
        pad = -len(payload) % 256
        off = self.size + BAND
        self.parts += [self._fill(BAND, kind, T), payload, self._fill(pad + BAND, kind, T)]
        self.at[name] = (off, len(payload), kind)
        self.size = off + len(payload) + pad + BAND

    def upload(self, torch):
        self.host = np.concatenate(self.parts)
        assert len(self.host) == self.size
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 256 == 0
        return self

    def ptr(self, name):
        return ctypes.c_void_p(self.dev.data_ptr() + self.at[name][0])

    def nbytes(self, name):
        return self.at[name][1]

    def download(self):
        """The device image; asserts that every byte outside the outputs and the workspace is as
        it was uploaded (the bands and the inputs)."""
        got = self.dev.cpu().numpy()
        keep = np.ones(self.size, dtype=bool)
        for off, n, kind in self.at.values():
            if kind != "in":
                keep[off:off + n] = False
        bad = np.nonzero((got != self.host) & keep)[0]
        if len(bad):
            where = [name for name, (off, n, _) in self.at.items()
                     if off - BAND <= bad[0] < off + n + 256 + BAND]
            raise AssertionError("%d bytes changed outside the outputs, first at %d (near %s)"
                                 % (len(bad), bad[0], where))
        self.got = got
        return self

    def out(self, name, T, shape):
        off, n, _ = self.at[name]
        return self.got[off:off + n].view(T).reshape(shape).copy()


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _finish(torch, rc):
    """Wait for the launch. A HIP error (a fault included) ends the session: nothing more is started
    on a device that has reported one."""
    from glx import _lib
    try:
        if rc != 2:   # GLX_E_HIP
            _lib.check(rc)
            torch.cuda.synchronize()
            return
        what = _lib.lib().glx_last_error().decode()
    except RuntimeError as e:
        if isinstance(e, _lib.GlxError):
            raise
        what = str(e)
    pytest.exit("HIP error, stopping: " + what, returncode=3)


def _ws_bytes(gdt, m, n, l):
    from glx import _lib
    nb = ctypes.c_size_t(0)
    _lib.check(_lib.lib().glx_kernel_workspace_bytes(gdt, m, n, l, ctypes.byref(nb)))
    return int(nb.value)


def run_ax(case, A, Xs, B):
    """R_s = A X_s - B for the case's right-hand sides: ([R_s], scalars) with scalars = [h] from
    glx_residual (one right-hand side) or sq[:nsrc] from glx_residual_batch; the four slots of sq
    are all the library's to write."""
    torch = _torch()
    from glx import _lib
    T = _np(case.dtype)
    gdt = _lib.GLX_F64 if case.dtype == "f64" else _lib.GLX_F32
    m, n, l, ns = case.m, case.n, case.l, case.nsrc
    es = np.dtype(T).itemsize
    ar = Arena()
    ar.add("A", "in", T, A)
    for s in range(ns):
        ar.add("X%d" % s, "in", T, Xs[s])
    ar.add("B", "in", T, B)
    for s in range(ns):
        ar.add("R%d" % s, "out", nbytes=m * l * es)
    ar.add("sc", "out", nbytes=8 if ns == 1 else 32)
    ar.add("ws", "ws", nbytes=_ws_bytes(gdt, m, n, l))
    ar.upload(torch)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if ns == 1:
        rc = _lib.lib().glx_residual(gdt, m, n, l, ar.ptr("A"), ar.ptr("X0"), ar.ptr("B"), ar.ptr("R0"),
                                     ar.ptr("sc"), ar.ptr("ws"), ar.nbytes("ws"), 0, st)
    else:
        xp = (ctypes.c_void_p * 3)(*[ar.ptr("X%d" % s) for s in range(ns)], *([None] * (3 - ns)))
        rp = (ctypes.c_void_p * 3)(*[ar.ptr("R%d" % s) for s in range(ns)], *([None] * (3 - ns)))
        rc = _lib.lib().glx_residual_batch(gdt, m, n, l, ar.ptr("A"), ns, xp, ar.ptr("B"), rp, ar.ptr("sc"),
                                           ar.ptr("ws"), ar.nbytes("ws"), 0, st)
    _finish(torch, rc)
    ar.download()
    Rs = [ar.out("R%d" % s, T, (m, l)) for s in range(ns)]
    sc = ar.out("sc", np.float64, (1 if ns == 1 else 4,))
    return Rs, sc[:ns]


def run_atr(case, A, R):
    torch = _torch()
    from glx import _lib
    T = _np(case.dtype)
    gdt = _lib.GLX_F64 if case.dtype == "f64" else _lib.GLX_F32
    m, n, l = case.m, case.n, case.l
    ar = Arena()
    ar.add("A", "in", T, A)
    ar.add("R", "in", T, R)
    ar.add("G", "out", nbytes=n * l * np.dtype(T).itemsize)
    ar.add("ws", "ws", nbytes=_ws_bytes(gdt, m, n, l))
    ar.upload(torch)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _finish(torch, _lib.lib().glx_gradient(gdt, m, n, l, ar.ptr("A"), ar.ptr("R"), ar.ptr("G"), ar.ptr("ws"),
                                           ar.nbytes("ws"), st))
    ar.download()
    return ar.out("G", T, (n, l))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------
# inputs and references (NumPy only; cached per shape and dtype, read-only)
# ---------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def int_ax(m, n, l):
    """Integer A, X_0..2, B and the int64 residuals."""
    assert n <= 2046
    i, k, j = np.arange(m)[:, None], np.arange(n), np.arange(l)
    A = (7 * i + 3 * k[None, :]) % 5 - 2
    Xs = [(5 * k[:, None] + 11 * j[None, :] + 3 * s) % 3 - 1 for s in range(3)]
    B = (3 * i + 5 * j[None, :]) % 7 - 3
    Rs = [A @ X - B for X in Xs]
    assert max(int(np.abs(R).max()) for R in Rs) ** 2 < 2 ** 24
    return _frozen(A, *Xs, B, *Rs)


@functools.lru_cache(maxsize=None)
def int_atr(m, n, l):
    i, k, j = np.arange(m)[:, None], np.arange(n), np.arange(l)
    A = (7 * i + 3 * k[None, :]) % 5 - 2
    R = (5 * i + 3 * j[None, :]) % 7 - 3
    return _frozen(A, R, A.T @ R)


def _scaled(rng, rows, cols):
    return rng.standard_normal((rows, cols)) * rng.choice([1e-3, 1.0, 30.0], size=(rows, 1))


@functools.lru_cache(maxsize=None)
def rnd_inputs(dtype, m, n, l):
    T = _np(dtype)
    rng = np.random.default_rng([m, n, l, 8 if dtype == "f64" else 4])
    A = _scaled(rng, m, n).astype(T)
    Xs = [_scaled(rng, n, l).astype(T) for _ in range(3)]
    B = rng.standard_normal((m, l)).astype(T)
    R = _scaled(rng, m, l).astype(T)
    return _frozen(A, *Xs, B, R)


@functools.lru_cache(maxsize=None)
def rnd_ax_ref(dtype, m, n, l, s):
    """(A X_s - B, the bar (n + 2) eps (|A||X_s| + |B|)) in the wider type."""
    T = _np(dtype)
    W = _wide(T)
    A, X, B = (rnd_inputs(dtype, m, n, l)[i].astype(W) for i in (0, 1 + s, 4))
    ref = A @ X - B
    bar = (n + 2) * W(np.finfo(T).eps) * (np.abs(A) @ np.abs(X) + np.abs(B))
    return _frozen(ref, bar)


@functools.lru_cache(maxsize=None)
def rnd_atr_ref(dtype, m, n, l):
    T = _np(dtype)
    W = _wide(T)
    A, R = (rnd_inputs(dtype, m, n, l)[i].astype(W) for i in (0, 5))
    return _frozen(A.T @ R, (m + 2) * W(np.finfo(T).eps) * (np.abs(A).T @ np.abs(R)))


def _assert_plan(case, monkeypatch):
    from glx import _lib
    tile_cases.apply_env(monkeypatch, case.env)
    plan = _lib.plan_describe(_lib.GLX_F64 if case.dtype == "f64" else _lib.GLX_F32, case.m, case.n, case.l)
    assert case.plan in plan.split("; "), (case.id, plan)


def _within(got, ref, bar, key):
    err = np.abs(got.astype(ref.dtype) - ref)
    ratio = float(np.max(err / np.maximum(bar, np.finfo(np.float64).tiny)))
    _note(key, ratio)
    assert np.all(err <= bar), (key, ratio)


# ---------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------
AX = [c for c in CASES if c.product == "ax"]
ATR = [c for c in CASES if c.product == "atr"]


@pytest.mark.parametrize("case", AX, ids=[c.id for c in AX])
def test_ax_tile(case, monkeypatch):
    _assert_plan(case, monkeypatch)
    T = _np(case.dtype)
    m, n, l, ns = case.m, case.n, case.l, case.nsrc
    scale = 0.5 if ns == 1 else 1.0   # glx_residual returns h = 0.5 sum r^2
    # (a) integers: equality
    ints = int_ax(m, n, l)
    A, Xs, B, refs = ints[0].astype(T), [x.astype(T) for x in ints[1:4]], ints[4].astype(T), ints[5:8]
    Rs, sc = run_ax(case, A, Xs, B)
    for s in range(ns):
        assert np.array_equal(Rs[s].astype(np.int64), refs[s]) and np.all(Rs[s] == np.rint(Rs[s])), (case.id, s)
        assert sc[s] == scale * float(np.sum(refs[s] * refs[s])), (case.id, s, sc[s])
    Rs2, sc2 = run_ax(case, A, Xs, B)
    assert all(_same_bits(a, b) for a, b in zip(Rs, Rs2)) and _same_bits(sc, sc2), case.id
    # (c) a NaN in A's last element: row m - 1 of every source, and every scalar
    An = A.copy()
    An[m - 1, n - 1] = np.nan
    Rn, scn = run_ax(case, An, Xs, B)
    for s in range(ns):
        assert np.isnan(Rn[s][m - 1]).all(), (case.id, s)
        assert _same_bits(Rn[s][:m - 1], Rs[s][:m - 1]), (case.id, s)
    assert np.isnan(scn).all(), (case.id, scn)
    # a NaN in one right-hand side: column l / 2 of that source (every row: 0 * NaN = NaN; the
    # rows with A[i, n - 1] != 0 first of all), its scalar, and nothing else
    sx, c = (1 if ns > 1 else 0), l // 2
    Xn = [x.copy() for x in Xs]
    Xn[sx][n - 1, c] = np.nan
    Rx, scx = run_ax(case, A, Xn, B)
    for s in range(ns):
        if s != sx:
            assert _same_bits(Rx[s], Rs[s]) and scx[s] == sc[s], (case.id, s)
    assert np.isnan(Rx[sx][A[:, n - 1] != 0, c]).all(), case.id
    assert np.isnan(Rx[sx][:, c]).all(), case.id
    keep = np.arange(l) != c
    assert _same_bits(Rx[sx][:, keep], Rs[sx][:, keep]), case.id
    assert np.isnan(scx[sx]), (case.id, scx)
    # (b) mixed scales against the wider type
    rnd = rnd_inputs(case.dtype, m, n, l)
    Rs, sc = run_ax(case, rnd[0], rnd[1:4], rnd[4])
    Rs2, sc2 = run_ax(case, rnd[0], rnd[1:4], rnd[4])
    assert all(_same_bits(a, b) for a, b in zip(Rs, Rs2)) and _same_bits(sc, sc2), case.id
    for s in range(ns):
        ref, bar = rnd_ax_ref(case.dtype, m, n, l, s)
        _within(Rs[s], ref, bar, "R " + case.dtype)
        ssq = np.sum(Rs[s].astype(np.longdouble) ** 2)
        sbar = (np.finfo(T).eps + D_SUM * np.finfo(np.float64).eps) * ssq
        ratio = float(abs(np.longdouble(sc[s]) - scale * ssq) / (scale * sbar))
        _note("h, sq " + case.dtype, ratio)
        assert ratio <= 1, (case.id, s, ratio)


@pytest.mark.parametrize("case", ATR, ids=[c.id for c in ATR])
def test_atr_tile(case, monkeypatch):
    _assert_plan(case, monkeypatch)
    T = _np(case.dtype)
    m, n, l = case.m, case.n, case.l
    # (a) integers: equality
    Ai, Ri, Gi = int_atr(m, n, l)
    A, R = Ai.astype(T), Ri.astype(T)
    G = run_atr(case, A, R)
    assert np.array_equal(G.astype(np.int64), Gi) and np.all(G == np.rint(G)), case.id
    assert _same_bits(G, run_atr(case, A, R)), case.id
    # (c) a NaN in R: column l / 2 of G (every row; the rows with A[m - 1, :] != 0 first of all)
    c = l // 2
    Rn = R.copy()
    Rn[m - 1, c] = np.nan
    Gn = run_atr(case, A, Rn)
    assert np.isnan(Gn[A[m - 1, :] != 0, c]).all(), case.id
    assert np.isnan(Gn[:, c]).all(), case.id
    keep = np.arange(l) != c
    assert _same_bits(Gn[:, keep], G[:, keep]), case.id
    # a NaN in A's last element: row n - 1 of G and nothing else
    An = A.copy()
    An[m - 1, n - 1] = np.nan
    Gn = run_atr(case, An, R)
    assert np.isnan(Gn[n - 1]).all(), case.id
    assert _same_bits(Gn[:n - 1], G[:n - 1]), case.id
    # (b) mixed scales against the wider type
    rnd = rnd_inputs(case.dtype, m, n, l)
    G = run_atr(case, rnd[0], rnd[5])
    assert _same_bits(G, run_atr(case, rnd[0], rnd[5])), case.id
    ref, bar = rnd_atr_ref(case.dtype, m, n, l)
    _within(G, ref, bar, "G " + case.dtype)
