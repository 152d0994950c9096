"""The fused A e walk of the dense pass (k_ax_dma EG, kernels_axdma.hip), one launch at a time
through glx.kernels.fused_ae_pass (glx_fused_ae_pass), with the tile forced by GLX_AX_VARIANT=92278.

Exact oracle, bit for bit: the kernel documents the order in which every (row, column) accumulator
of a K split's A e slab receives its entries: the row block's (rotated) walk over the split's
32-column chunks, ascending k inside a chunk, one rounded multiply and one rounded add per entry.
From the returned S and rotation flag the host repeats exactly that in NumPy float64 and the slabs
must agree in every bit. The sum of the slabs is also set against float64 A @ e within
1e-13 max|A| ||e_c||_1 per column, which guards the oracle itself.

The A p slabs of the same launch (MFMA) are checked against A @ p within the a-priori bound of two
recursive sums of n + S terms: 2 (n + S) 2^-53 max|A| ||p_c||_1 per column.

Shapes are the smallest that reach each path of the pipelined loop (one chunk and the odd-count
tail; three chunks at l = 16; two row blocks with a ragged last row; three K splits with the chunk
rotation on; the planner's own S and XCD map), each with every entry pattern.
"""
import functools
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

THRES = 1e-3
TILE_ROWS = 256   # rows of a workgroup of tile 92278 (8 waves x 2 row tiles x 16)
KC = 32           # columns of a chunk

# (m, n, l, S, GLX_AX_S or None)
SHAPES = [
    (17, 32, 32, 1, None),
    (17, 96, 16, 1, None),
    (257, 160, 32, 1, None),
    (257, 800, 16, 3, "3"),
    (512, 2048, 32, 8, None),
]
PATTERNS = ["none", "first", "last", "chunk_edge", "dense_chunk", "full_column", "random"]


def _ids(s):
    return "%dx%dx%d_S%d" % s[:4]


@functools.lru_cache(maxsize=None)
def _matrix(m, n):
    rng = np.random.default_rng(1000 * m + n)
    A = rng.standard_normal((m, n))
    return A, torch.from_numpy(A).cuda()


def _flags(pattern, n, l):
    f = np.zeros((n, l), dtype=bool)
    if pattern == "first":
        f[0, 0] = True
    elif pattern == "last":
        f[n - 1, l - 1] = True
    elif pattern == "chunk_edge":   # neighbours across a chunk edge (k = 32 where n has it)
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


def _env(monkeypatch, ax_s):
    monkeypatch.setenv("GLX_AX_VARIANT", "92278")
    if ax_s is None:
        monkeypatch.delenv("GLX_AX_S", raising=False)
    else:
        monkeypatch.setenv("GLX_AX_S", ax_s)


def _launch(A_d, p):
    from glx import kernels
    out = kernels.fused_ae_pass(A_d, torch.from_numpy(p).cuda(), THRES)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_ae_slabs_bit_exact(monkeypatch, shape, pattern):
    m, n, l, S, ax_s = shape
    _env(monkeypatch, ax_s)
    A, A_d = _matrix(m, n)
    p, f = _candidate(pattern, n, l)
    out = _launch(A_d, p)
    assert out["S"] == S
    if S == 3:
        assert out["rotated"], "the three-split case is there for the rotated walk"
    e = np.where(f, p, 0.0)
    assert np.array_equal(out["e"].cpu().numpy(), e)   # exactly the pattern's entries are flagged
    Pe = out["Pe"].cpu().numpy()
    ref = _oracle_pe(A, e, out["S"], out["rotated"])
    # the oracle itself, against the plain product
    amax = np.max(np.abs(A))
    bound = 1e-13 * amax * np.sum(np.abs(e), axis=0)
    err = np.max(np.abs(ref.sum(axis=0) - A @ e), axis=0)
    print("oracle vs A @ e: max err / bound per column", np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound)
    same = Pe.view(np.int64) == ref.view(np.int64)
    print("A e slabs: %d of %d values differ in bits" % (same.size - int(same.sum()), same.size))
    assert np.array_equal(Pe.view(np.int64), ref.view(np.int64))
    # the A p slabs of the same launch
    P = out["P"].cpu().numpy().sum(axis=0)
    pb = 2.0 * (n + S) * 2.0 ** -53 * amax * np.sum(np.abs(p), axis=0)
    perr = np.max(np.abs(P - A @ p), axis=0)
    print("A p: max err / bound per column", np.max(perr / pb))
    assert np.all(perr <= pb)


def test_run_to_run_identical_bits(monkeypatch):
    m, n, l, S, ax_s = SHAPES[-1]
    _env(monkeypatch, ax_s)
    A, A_d = _matrix(m, n)
    p, _ = _candidate("random", n, l)
    a, b = _launch(A_d, p), _launch(A_d, p)
    for key in ("P", "Pe"):
        assert np.array_equal(a[key].cpu().numpy().view(np.int64), b[key].cpu().numpy().view(np.int64)), key


def test_hybrid_session_counts_both_forms_and_matches_oracle(monkeypatch):
    """3 x 10 iterations at (1024, 16384, 32), the switch forced early (50 flagged rows): both
    forms run, and the solve meets the bars of tests/test_gpu_egat.py against the oracle."""
    from glx.solver import Session
    from oracle import numpy_ref
    m, n, l, maxit = 1024, 16384, 32, 10
    monkeypatch.setenv("GLX_AX_VARIANT", "92278")
    monkeypatch.setenv("GLX_AE_HYB_ROWS", "50")
    monkeypatch.delenv("GLX_AE_FUSED", raising=False)
    monkeypatch.delenv("GLX_AX_S", raising=False)
    A, b, u, x0, mu = numpy_ref.gen_data(m, n, l, 97006855)
    opts = {"alpha0": numpy_ref.step_size_for(m, n), "maxit": maxit}
    xd = torch.from_numpy(x0).cuda().clone()
    s = Session("gl_ProxGD_primal", xd, torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), float(mu),
                dict(opts))
    try:
        plan = s.describe()
        s.run(0)
        res = s.finish()
        cnt = s.ae_forms()
    finally:
        s.close()
    torch.cuda.synchronize()
    print(plan)
    print(cnt)
    assert "from 50 flagged rows" in plan, plan
    assert cnt["ae_gather_trials"] > 0 and cnt["ae_fused_trials"] > 0, cnt
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xr, kr, outr = numpy_ref.gl_ProxGD_primal(x0, A, b, mu, dict(opts))
    fr = np.asarray([float(v) for v in outr["f_hist"]])
    fh = np.asarray([float(v) for v in res["f_hist"]])
    x = xd.cpu().numpy()
    assert res["k"] == kr == 3 * maxit
    assert np.max(np.abs(fh - fr) / np.abs(fr)) < 1e-8
    assert np.max(np.abs(x - xr)) <= 1e-6 * np.max(np.abs(xr))
