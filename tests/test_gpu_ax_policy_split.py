"""The dense pass's pipelined loop split by load policy (k_ax_dma, kernels_axdma.hip), one launch at
a time through glx.kernels.dense_pass_keep (glx_dense_pass_keep), tile forced by GLX_AX_VARIANT=92278.

With a keep size the walk of a block runs as trips that issue (non-temporal, non-temporal), at most
one mixed trip, then (default, default) trips; the stand-alone entries of tests/test_gpu_ae_walk.py
plan with a keep size of 0 and reach only the first kind. A walk step of the grid is grid x 64 KiB
(8 waves x 8 KiB of A per block and chunk), so a block's first default-policy step is
kt = nch - keep 2^20 / (grid 65536):

  (512, 2048, 32): S 8, grid 16, nch 8; keep {0, 1, 3, 4, 7, 8, 100} -> kt {8, 7, 5, 4, 1, 0, < 0}: all
      non-temporal, an odd and an even split point, the mixed trip, all default, a negative kt;
  (257, 800, 16): S 3 (GLX_AX_S=3), rotated, grid 6, nch 8, 8, 9; keep {0, 1, 2, 3}: both parities of
      nch cross the split;
  (17, 32, 32) and (17, 96, 16): nch 1 and 3, keep {0, 1}: the prologue alone and the odd-count tail.

The load policy changes no arithmetic, so for every keep size, plain and fused: the A p slabs have the
bits of the keep = 0 launch and the same bits plain and fused, and lie within the a-priori bound of
tests/test_gpu_ae_walk.py (2 (n + S) 2^-53 max|A| ||p_c||_1 per column); the A e slabs have the bits
of that file's host oracle (repeated here): the row block's (rotated) walk over the split's chunks,
ascending k inside a chunk, one rounded multiply and one rounded add per entry; and a launch made
twice gives the same bits. One session of 30 iterations (GLX_AE_HYB_ROWS=1) must not depend on
GLX_AX_KEEP_MIB in any byte of x and f_hist.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

THRES = 1e-3
TILE_ROWS = 256   # rows of a workgroup of tile 92278 (8 waves x 2 row tiles x 16)
KC = 32           # columns of a chunk

# (m, n, l, S, GLX_AX_S or None, keep sizes in MiB)
SHAPES = [
    (512, 2048, 32, 8, None, (0, 1, 3, 4, 7, 8, 100)),
    (257, 800, 16, 3, "3", (0, 1, 2, 3)),
    (17, 32, 32, 1, None, (0, 1)),
    (17, 96, 16, 1, None, (0, 1)),
]
PATTERNS = ["none", "chunk_edge", "dense_chunk", "full_column", "random"]


def _ids(s):
    return "%dx%dx%d_S%d" % s[:4]


@functools.lru_cache(maxsize=None)
def _matrix(m, n):
    rng = np.random.default_rng(1000 * m + n)
    A = rng.standard_normal((m, n))
    return A, torch.from_numpy(A).cuda()


def _flags(pattern, n, l):
    f = np.zeros((n, l), dtype=bool)
    if pattern == "chunk_edge":     # neighbours across a chunk edge (k = 32 where n has it)
        for k in (31, 32):
            if k < n:
                f[k, 3] = True
                f[k, l - 2] = True
    elif pattern == "dense_chunk":  # every entry of one chunk: the densest bitmap words
        c = (n // KC) // 2
        f[KC * c:KC * (c + 1), :] = True
    elif pattern == "full_column":
        f[:, l // 2 + 1] = True
    elif pattern == "random":
        f = np.random.default_rng(20240607).random((n, l)) < 0.02
    return f


def _candidate(pattern, n, l):
    """p with exactly the pattern's entries below THRES and nonzero."""
    rng = np.random.default_rng(7 + n + l)
    sign = np.where(rng.random((n, l)) < 0.5, -1.0, 1.0)
    p = sign * rng.uniform(0.5, 1.5, (n, l))                      # |p| >= 0.5: kept
    small = sign * rng.uniform(0.1, 0.9, (n, l)) * THRES          # 0 < |p| < THRES: flagged
    f = _flags(pattern, n, l)
    return np.where(f, small, p), f


def _oracle_pe(A, e, S, rotated):
    """The A e slabs in the kernel's order of summation."""
    m, n = A.shape
    l = e.shape[1]
    chunks = n // KC
    gx = -(-m // TILE_ROWS)
    Pe = np.zeros((S, m, l))
    nzrows = [np.flatnonzero(e[k]) for k in range(n)]
    for by in range(S):
        cb, ce = chunks * by // S, chunks * (by + 1) // S
        nch = ce - cb
        for bx in range(gx):
            r0, r1 = bx * TILE_ROWS, min(m, (bx + 1) * TILE_ROWS)
            rot = (bx * nch) // gx if rotated else 0
            acc = Pe[by, r0:r1]
            for step in range(nch):
                c = step + rot
                c = c - nch if c >= nch else c
                for k in range(KC * (cb + c), KC * (cb + c + 1)):
                    cols = nzrows[k]
                    if cols.size:
                        prod = A[r0:r1, k][:, None] * e[k, cols][None, :]   # one rounded multiply
                        acc[:, cols] = acc[:, cols] + prod                  # one rounded add
    return Pe


@functools.lru_cache(maxsize=None)
def _reference(m, n, l, pattern, S, rotated):
    """(p, e, the oracle's A e slabs, A @ p, the A p bound per column): once per shape and pattern."""
    A, _ = _matrix(m, n)
    p, f = _candidate(pattern, n, l)
    e = np.where(f, p, 0.0)
    ref = _oracle_pe(A, e, S, rotated)
    amax = np.max(np.abs(A))
    # the oracle itself, against the plain product
    bound = 1e-13 * amax * np.sum(np.abs(e), axis=0)
    assert np.all(np.max(np.abs(ref.sum(axis=0) - A @ e), axis=0) <= bound)
    pb = 2.0 * (n + S) * 2.0 ** -53 * amax * np.sum(np.abs(p), axis=0)
    for a in (p, e, ref):
        a.setflags(write=False)
    return p, e, ref, A @ p, pb


def _env(monkeypatch, ax_s):
    monkeypatch.setenv("GLX_AX_VARIANT", "92278")
    if ax_s is None:
        monkeypatch.delenv("GLX_AX_S", raising=False)
    else:
        monkeypatch.setenv("GLX_AX_S", ax_s)


def _bits(t):
    return t.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_keep_size_changes_no_bit(monkeypatch, shape, pattern):
    from glx import kernels
    m, n, l, S, ax_s, keeps = shape
    _env(monkeypatch, ax_s)
    _, A_d = _matrix(m, n)
    p0, _ = _candidate(pattern, n, l)
    p_d = torch.from_numpy(p0).cuda()
    base = None
    for keep in keeps:
        runs = {}
        for fused in (True, False):
            a = kernels.dense_pass_keep(A_d, p_d, keep, fused, THRES)
            b = kernels.dense_pass_keep(A_d, p_d, keep, fused, THRES)
            torch.cuda.synchronize()
            assert a["S"] == S
            if S == 3:
                assert a["rotated"], "the three-split case is there for the rotated walk"
            for key in ("P", "Pe") if fused else ("P",):
                assert np.array_equal(_bits(a[key]), _bits(b[key])), (keep, fused, key, "run to run")
            runs[fused] = a
        out = runs[True]
        p, e, ref, Ap, pb = _reference(m, n, l, pattern, out["S"], out["rotated"])
        assert np.array_equal(out["e"].cpu().numpy(), e)   # exactly the pattern's entries are flagged
        P = _bits(out["P"])
        if base is None:
            base = P   # keep = 0, the first of every list
        assert np.array_equal(P, base), (keep, "A p against keep = 0")
        assert np.array_equal(_bits(runs[False]["P"]), P), (keep, "A p plain against fused")
        perr = np.max(np.abs(out["P"].cpu().numpy().sum(axis=0) - Ap), axis=0)
        print("keep %d: A p max err / bound per column %.3g" % (keep, np.max(perr / pb)))
        assert np.all(perr <= pb), keep
        Pe = _bits(out["Pe"])
        diff = int((Pe != ref.view(np.int64)).sum())
        print("keep %d: A e slabs: %d of %d values differ in bits" % (keep, diff, Pe.size))
        assert diff == 0, keep


def test_session_does_not_depend_on_keep_size(monkeypatch):
    """30 iterations at (512, 2048, 32), GLX_AE_HYB_ROWS=1 (a split-candidate trial, where one comes,
    takes the fused form): x and f_hist byte for byte the same with GLX_AX_KEEP_MIB = 0, 3 and unset.
    The trial counts are printed; a solve this short may meet no split candidate, and then it is the
    plain pass that runs under the three keep sizes."""
    from glx.solver import Session
    from oracle import numpy_ref
    m, n, l, maxit = 512, 2048, 32, 10
    monkeypatch.setenv("GLX_AX_VARIANT", "92278")
    monkeypatch.setenv("GLX_AE_HYB_ROWS", "1")
    monkeypatch.delenv("GLX_AE_FUSED", raising=False)
    monkeypatch.delenv("GLX_AX_S", raising=False)
    A, b, u, x0, mu = numpy_ref.gen_data(m, n, l, 97006855)
    A_d, b_d = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
    opts = {"alpha0": numpy_ref.step_size_for(m, n), "maxit": maxit}
    got = {}
    for keep in ("0", "3", None):
        if keep is None:
            monkeypatch.delenv("GLX_AX_KEEP_MIB", raising=False)
        else:
            monkeypatch.setenv("GLX_AX_KEEP_MIB", keep)
        xd = torch.from_numpy(x0).cuda().clone()
        s = Session("gl_ProxGD_primal", xd, A_d, b_d, float(mu), dict(opts))
        try:
            s.run(0)
            res = s.finish()
            cnt = s.ae_forms()
        finally:
            s.close()
        torch.cuda.synchronize()
        print(keep, res["k"], cnt)
        assert res["k"] == 3 * maxit
        got[keep] = (xd.cpu().numpy().tobytes(), np.asarray(res["f_hist"], dtype=np.float64).tobytes())
    assert got["0"] == got["3"] == got[None]
