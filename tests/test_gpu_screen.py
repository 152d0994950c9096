"""Gap-safe screening on the GPU: the three kernels one launch at a time, whole certified solves,
the path over mu and the refusals. Reference: tests/screen_ref.py.

1. Column norms (glx.kernels.col_norms). The reference is longdouble on the float64 values the
   input was rounded from. Bar: a column's m squares (exact in double for float32 inputs, one
   rounding each for float64) and m - 1 additions give the sum a relative error of at most
   (m + 1) u64, the root halves it and rounds once: (m + 2) eps64 / 2 relative, u64 = eps64 / 2, so
   the bar has a factor 2 in hand; the input's rounding adds eps32 / 2 relative for float32. The
   maximum is that of the returned norms, bit for bit; the sum of squares is within
   (m + n + 2) eps64 relative. Both bars are functions of the shape, so they hold as they stand past
   the grid's cap of 1024 column blocks (n = 262214: a second column for 70 lanes, one trip more) and
   at 64 slabs (m = 4097).
2. The screen step (glx.kernels.screen_step) on synthetic norms with margins set by construction:
   row i sits at lhs_i = mu (1 + sign_i d_i), d_i in [1e-6, 0.5], so the GPU's three roundings in
   double (~4e-16 relative) cannot flip it; at most 8 rows are placed within one ulp of the
   threshold and are exempt from the mask comparison (only they may differ). n = 16385 and 16449
   give the list builder's threads two ballot words each (the last ones one or none), n = 262209 a
   second trip of two waves past the 1024-workgroup cap and 17 words a thread.
3. The gather (glx.kernels.gather_cols): bit-equal to A[:, idx], pad columns exactly 0, canaries.
   m = 1030 and 5123 at 64 destination columns make the 1024 row walkers read a second row and a
   whole unrolled group of four; wp = 576 / 1088 give a second block of column groups.
4. Whole solves against a reference solved to rel_gap <= 1e-12 (screen_ref.reference_solution).
   Slack of the objective comparisons: the reference's own gap plus screen_ref.primal_bar, the
   rounding of a primal value composed from a record in A's dtype (the guard's item 2).
5. The path. "Kept" is info["kept"], the rows the last screening test of a solve did not prove zero
   (the first entry stops at its first check with no compaction, so its reduced width is still n).
6. Refusals.
"""
import functools

import numpy as np
import pytest

import certificate_ref as cref
import screen_ref as sr

pytestmark = pytest.mark.gpu

EPS64 = sr.EPS64
SEED = 1   # the seed of the issue's NumPy model


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(a, dtype=None):
    torch = _torch()
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else \
        torch.as_tensor(np.ascontiguousarray(a).astype(dtype), device="cuda")


# ------------------------------------------------------------------------------------------ 1
def _col_norms_case(dt, m, n, g):
    from glx import kernels
    A64 = g.standard_normal((m, n))
    A64[:, n // 2] *= 1e-3
    if n > 2:
        A64[:, 1] = 0.0
    want = sr.col_norms(A64)
    Ad = _dev(A64, dt)
    norms, stats = kernels.col_norms(Ad)
    got = norms.cpu().numpy()
    st = stats.cpu().numpy()
    bar = ((m + 2) * EPS64 / 2 + (sr.EPS32 / 2 if dt == np.float32 else 0.0)) * want
    err = np.abs(got.astype(sr.LD) - want)
    assert np.all(err <= bar), (m, n, float(np.max(err / np.maximum(bar, 1e-300))))
    assert st[0] == got.max()
    sq = float(np.sum(got.astype(sr.LD) ** 2))
    assert abs(st[1] - sq) <= (m + n + 2) * EPS64 * sq
    norms2, stats2 = kernels.col_norms(Ad)
    assert np.array_equal(norms2.cpu().numpy(), got) and np.array_equal(stats2.cpu().numpy(), st)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_col_norms(dt):
    g = np.random.default_rng(11)
    shapes = [(m, n) for m in (1, 63, 64, 257) for n in (1, 63, 64, 65, 200)] + [(130, 600)]
    for m, n in shapes:
        _col_norms_case(dt, m, n, g)


# (m, 262214): 70 columns past the 1024-workgroup cap, so the first 70 lanes of workgroup 0 walk a
# second column, in one slab (m = 3) and in three (m = 130); (4097, 70): 64 slabs of 65 rows, the last
# of two. The bars are those of test 1: they grow with m, and the stats' with m + n.
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("m,n", [(3, 262214), (130, 262214), (4097, 70)])
def test_col_norms_several_trips(m, n, dt):
    _col_norms_case(dt, m, n, np.random.default_rng(11 + m + n))


def test_col_norms_nan_reaches_the_maximum():
    from glx import kernels
    A = np.ones((5, 70))
    A[3, 68] = np.nan
    norms, stats = kernels.col_norms(_dev(A))
    got = norms.cpu().numpy()
    assert np.isnan(got[68]) and np.all(got[np.arange(70) != 68] == np.sqrt(5.0))
    assert np.isnan(stats.cpu().numpy()[0])


# ------------------------------------------------------------------------------------------ 2
MU, S, RHO = 1.0, 0.7, 0.05


def _synthetic(n, kind, seed):
    """(row norms, column norms, the intended keep mask, the rows within one ulp of the threshold)."""
    g = np.random.default_rng(seed)
    cn = g.uniform(0.5, 2.0, n)
    if kind == "all":
        keep = np.ones(n, dtype=bool)
    elif kind == "none":
        keep = np.zeros(n, dtype=bool)
    elif kind == "one":
        keep = np.zeros(n, dtype=bool)
        keep[int(g.integers(n))] = True
    else:
        keep = g.random(n) < 0.4
    d = g.uniform(1e-6, 0.5, n)
    d[: min(n, 3)] = 1e-6                         # some rows exactly at the smallest margin
    lhs = MU * (1.0 + np.where(keep, d, -d))
    rn = (lhs - cn * RHO) / S
    assert np.all(rn > 0)
    near = np.zeros(n, dtype=bool)
    if kind == "random" and n >= 64:
        at = g.choice(n, size=8, replace=False)
        near[at] = True
        rn[at] = (MU - cn[at] * RHO) / S
        rn[at[::2]] = np.nextafter(rn[at[::2]], np.inf)
    return rn, cn, keep, near


def _check_list(out, n):
    mask = out["mask"].cpu().numpy()
    lst = out["list"].cpu().numpy()
    cnt = out["count"].cpu().numpy()
    assert set(np.unique(mask)) <= {0, 1}
    want = np.nonzero(mask)[0]
    kept, wp = int(cnt[0]), int(cnt[1])
    assert kept == want.size and wp == (kept + 63) // 64 * 64
    assert np.array_equal(lst[:kept], want)
    assert np.all(lst[kept:wp] == -1)
    assert np.all(lst[wp:] == -2)                 # nothing written past the padded width
    return mask.astype(bool)


# (16385 and 16449: the list builder's 256 threads take two ballot words each, the last ones one or
# none; 262209: past the 1024-workgroup cap, two waves make a second trip, and 17 words a thread)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097, 16385, 16449, 262209])
def test_screen_step(n):
    from glx import kernels
    for kind in ("random", "all", "none", "one"):
        rn, cn, keep, near = _synthetic(n, kind, 100 + n)
        ref = sr.keep_mask(rn, cn, S, RHO, MU)
        assert near.sum() <= 8 and np.array_equal(ref[~near], keep[~near])   # the reference meets the condition
        out = kernels.screen_step(_dev(rn), _dev(cn), S, RHO, MU)
        mask = _check_list(out, n)
        assert np.array_equal(mask[~near], ref[~near]), (n, kind)
        again = kernels.screen_step(_dev(rn), _dev(cn), S, RHO, MU)
        for key in ("mask", "list", "count"):
            assert np.array_equal(again[key].cpu().numpy(), out[key].cpu().numpy()), (n, kind, key)


def test_screen_step_nan_keeps_the_row():
    from glx import kernels
    n = 200
    rn, cn, keep, _ = _synthetic(n, "none", 5)
    rn[[0, 63, 64, 199]] = np.nan
    cn2 = cn.copy()
    cn2[100] = np.nan
    mask = _check_list(kernels.screen_step(_dev(rn), _dev(cn2), S, RHO, MU), n)
    assert np.array_equal(np.nonzero(mask)[0], [0, 63, 64, 100, 199])
    for s, rho, mu in ((np.nan, RHO, MU), (S, np.nan, MU), (S, RHO, np.nan)):
        mask = _check_list(kernels.screen_step(_dev(rn), _dev(cn), s, rho, mu), n)
        assert mask.all()


# ------------------------------------------------------------------------------------------ 3
def _padded(idx):
    wp = (len(idx) + 63) // 64 * 64
    out = np.full(wp, -1, dtype=np.int32)
    out[: len(idx)] = idx
    return out


def _gather_case(g, dt, aligned, m, sw, kept):
    from glx import kernels
    torch = _torch()
    tdt = torch.float64 if dt == np.float64 else torch.float32
    canary = -7.25
    A = g.standard_normal((m, sw)).astype(dt)
    Ad = _dev(A)
    idx = np.sort(g.choice(sw, size=kept, replace=False)).astype(np.int32)
    pidx = _padded(idx)
    wp = len(pidx)
    off = 0 if aligned else 1
    flat = torch.full((off + m * wp + 64,), canary, dtype=tdt, device="cuda")
    out = flat[off: off + m * wp].view(m, wp)
    kernels.gather_cols(Ad, _dev(pidx), out=out)
    got = flat.cpu().numpy()
    body = got[off: off + m * wp].reshape(m, wp)
    assert np.array_equal(body[:, :kept], A[:, idx]), (m, sw, kept)
    assert np.all(body[:, kept:] == 0) and not np.any(np.signbit(body[:, kept:]))
    assert np.all(got[:off] == canary) and np.all(got[off + m * wp:] == canary)
    if kept >= 63:   # second generation: buffer to buffer, a list of the first one's columns
        idx2 = np.sort(g.choice(kept, size=kept // 2, replace=False)).astype(np.int32)
        p2 = _padded(idx2)
        src = out.contiguous()
        got2 = kernels.gather_cols(src, _dev(p2)).cpu().numpy()
        assert np.array_equal(got2[:, : len(idx2)], A[:, idx[idx2]])
        assert np.all(got2[:, len(idx2):] == 0)


# A row walk: wp = 64 is one block of column groups and 1024 row walkers, so at m = 1030 six of
# them read a second row and at m = 5123 each reads five or six (one unrolled group of four, then the
# rest). Two blocks of column groups: a thread stores 16 bytes where dst is aligned and one value
# elsewhere, so wp = 576 (f64, 2 a thread) / 1088 (f32, 4 a thread; f64 unaligned: 5 blocks), the
# second block partly past wp.
GATHER_LARGE = {(np.float64, True): [(1030, 100, 60), (5123, 100, 60), (830, 1200, 570)],
                (np.float64, False): [(1030, 100, 60), (5123, 100, 60), (830, 1200, 1080)],
                (np.float32, True): [(1030, 100, 60), (5123, 100, 60), (830, 1200, 1080)],
                (np.float32, False): [(1030, 100, 60), (5123, 100, 60)]}


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "unaligned"])
def test_gather_cols(dt, aligned):
    g = np.random.default_rng(3)
    for m in (1, 17, 256):
        for sw in (65, 512):
            for kept in (0, 1, 63, 64, 65):
                _gather_case(g, dt, aligned, m, sw, kept)
    for m, sw, kept in GATHER_LARGE[(dt, aligned)]:
        _gather_case(g, dt, aligned, m, sw, kept)


# ------------------------------------------------------------------------------------------ 4
CASES = [(96, 512, 16, 0.5), (96, 512, 16, 0.1), (40, 130, 3, 0.1)]
TOL = 1e-8


@functools.lru_cache(maxsize=None)
def _solved(m, n, l, ratio, screen, f32=False, tol=TOL):
    import glx
    ref = sr.reference_solution(SEED, m, n, l, ratio, f32)
    dt = np.float32 if f32 else np.float64
    x, info = glx.solve_certified(ref["A"].astype(dt), ref["b"].astype(dt), ref["mu"], tol=tol, screen=screen)
    return x, info


def _assert_safe(ref, info, n):
    screened = np.ones(n, dtype=bool)
    screened[info["kept_rows"]] = False
    assert screened.sum() == n - len(info["kept_rows"])
    bad = np.nonzero(screened & ~(ref["gtheta"] < sr.LD(ref["mu"])))[0]
    assert bad.size == 0, ("screened rows that are active at the reference solution", bad[:10])
    assert not np.any(screened & (np.sqrt(np.sum(ref["x"] ** 2, axis=1)) != 0))
    return screened


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d@%g" % c)
def test_certified_solve_f64(case):
    import glx
    from glx.certificate import record
    m, n, l, ratio = case
    ref = sr.reference_solution(SEED, m, n, l, ratio)
    A, b, mu = ref["A"].copy(), ref["b"].copy(), ref["mu"]   # (the shared arrays are read-only)
    x, info = _solved(m, n, l, ratio, True)
    xu, infou = _solved(m, n, l, ratio, False)
    print("\n%s: screened arm %d iterations, %d compactions %s, kept %d, width %d, passes %.1f, rel_gap %.2e; "
          "unscreened %d iterations, passes %.1f, rel_gap %.2e; reference rel_gap %.2e"
          % (case, info["iterations"], info["compactions"], info["kept_history"], info["kept"], info["width"],
             info["passes"], info["rel_gap"], infou["iterations"], infou["passes"], infou["rel_gap"],
             float(ref["gap"] / ref["primal"])))
    assert info["converged"] and infou["converged"]
    assert info["rel_gap"] <= TOL and infou["rel_gap"] <= TOL
    # the returned certificate is glx.certificate's of the returned x on the full problem
    cert = glx.certificate(x, A, b, mu)
    for key in ("primal", "dual", "gap", "rel_gap", "scale", "gmax", "kkt_max", "kkt_fro", "nonzero_rows"):
        assert info[key] == cert[key], key
    assert info["compactions"] >= 1 and info["width"] < n and info["kept"] < n
    assert info["kept_history"] == sorted(info["kept_history"], reverse=True)
    assert infou["compactions"] == 0 and infou["width"] == n
    assert info["passes"] < infou["passes"]
    _assert_safe(ref, info, n)
    P = float(ref["primal"])
    assert abs(info["primal"] - infou["primal"]) <= 2 * TOL * P
    cn = np.asarray(sr.col_norms(A), dtype=np.float64)
    for xx, ii in ((x, info), (xu, infou)):
        slack = float(ref["gap"]) + sr.primal_bar(record(xx, A, b, mu), mu, EPS64, m, n, l, float(np.sum(cn * cn)),
                                                  float(np.linalg.norm(b)))
        assert slack <= 1e-10 * P
        assert ii["primal"] >= float(ref["dual"]) - slack           # P(x) >= P* >= D_ref
        assert ii["primal"] - ii["gap"] <= P + slack                # D(theta) <= P* <= P_ref


def test_certified_solve_f32():
    m, n, l, ratio = 96, 512, 16, 0.5
    ref = sr.reference_solution(SEED, m, n, l, ratio, True)
    x, info = _solved(m, n, l, ratio, True, True, 1e-4)
    print("\nf32: %d iterations, compactions %s, kept %d, rel_gap %.2e"
          % (info["iterations"], info["kept_history"], info["kept"], info["rel_gap"]))
    assert x.dtype == np.float32
    assert info["converged"]
    _assert_safe(ref, info, n)


def test_warm_start_and_tensor_inputs():
    import glx
    torch = _torch()
    m, n, l, ratio = 40, 130, 3, 0.1
    ref = sr.reference_solution(SEED, m, n, l, ratio)
    x, info = _solved(m, n, l, ratio, True)
    x0 = torch.as_tensor(x, device="cuda")
    keep = x0.clone()
    xt, it = glx.solve_certified(torch.as_tensor(ref["A"].copy(), device="cuda"),
                                 torch.as_tensor(ref["b"].copy(), device="cuda"),
                                 ref["mu"], x0=x0, tol=TOL)
    assert isinstance(xt, torch.Tensor) and torch.equal(x0, keep)
    assert it["converged"] and it["iterations"] == 0 and it["checks"] == 1
    assert np.array_equal(xt.cpu().numpy(), x)


# ------------------------------------------------------------------------------------------ 5
def test_path():
    import glx
    m, n, l = 96, 512, 16
    A, b, _, _ = cref.instance(SEED, m, n, l)
    tol = 1e-6
    out = glx.path(A, b, n_mus=4, mu_min_ratio=0.05, tol=tol)
    assert len(out) == 4
    mus = [o[0] for o in out]
    assert mus[0] == glx.mu_max(A, b) and all(b_ < a_ for a_, b_ in zip(mus, mus[1:]))
    assert abs(mus[-1] - 0.05 * mus[0]) <= 1e-12 * mus[0]
    mu0, x0, i0 = out[0]
    assert np.all(x0 == 0) and i0["iterations"] == 0 and i0["gap"] == 0.0 and i0["converged"]
    kept = [o[2]["kept"] for o in out]
    print("\npath: mu / mu_max %s, kept %s, iterations %s" % ([round(v / mus[0], 4) for v in mus], kept,
                                                               [o[2]["iterations"] for o in out]))
    for mu, x, info in out:
        assert info["converged"] and info["rel_gap"] <= tol and info["mu"] == mu
        assert x.shape == (n, l)
    assert kept == sorted(kept)
    warm = sum(o[2]["iterations"] for o in out)
    cold = sum(glx.solve_certified(A, b, mu, tol=tol)[1]["iterations"] for mu in mus)
    print("warm-started %d iterations, cold %d" % (warm, cold))
    assert warm < cold
    same = glx.path(A, b, mus=mus[:2], tol=tol)
    assert np.array_equal(same[1][1], out[1][1])


# ------------------------------------------------------------------------------------------ 6
def test_refusals():
    import glx
    from glx import _lib
    A, b, _, _ = cref.instance(SEED, 40, 130, 3)
    with pytest.raises(ValueError):
        glx.solve_certified(A, b, 0.1, comm=object())
    with pytest.raises(ValueError):
        glx.path(A, b, comm=object())
    with pytest.raises(ValueError):
        glx.solve_certified(A, b, -0.1)
    with pytest.raises(ValueError):
        glx.solve_certified(A, b[:-1], 0.1)
    with pytest.raises(ValueError):
        glx.solve_certified(A, b, 0.1, x0=np.zeros((129, 3)))
    with pytest.raises(_lib.GlxError, match="l <= 128"):
        glx.solve_certified(A, np.zeros((40, 129)), 0.1)
    # the C entry itself refuses a communicator (the Python layer never passes one)
    import ctypes
    torch = _torch()
    Ad, bd = _dev(A), _dev(b)
    xd = torch.zeros((130, 3), dtype=torch.float64, device="cuda")
    nb = ctypes.c_size_t(0)
    _lib.check(_lib.lib().glx_certified_workspace_bytes(_lib.GLX_F64, 40, 130, 3, 1, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    info = _lib.GlxCertifiedInfo()
    p = _lib.GlxProblem(dtype=_lib.GLX_F64, method=0, m=40, n=130, l=3, A=Ad.data_ptr(), b=bd.data_ptr(),
                        x=xd.data_ptr(), mu0=0.1, comm=ws.data_ptr())
    rc = _lib.lib().glx_certified_solve(ctypes.byref(p), 1e-3, 1e-6, 10, 1, 10, None, None, None, ws.data_ptr(),
                                        ws.numel(), ctypes.byref(info), None)
    assert rc == 1 and b"single-GPU" in _lib.lib().glx_last_error()
    assert torch.count_nonzero(xd).item() == 0


# ------------------------------------------------------------------------------------------ driver
def test_driver_certified_rows():
    """python -m glx.driver --certified: the solvers' rows are what they are without the flag, one
    "Certified" row (or the path's ten) follows them."""
    import io
    from glx import driver
    fake = {"Fake": lambda x0, A, b, mu, opts: (np.zeros_like(x0), 3, {"tt": 0.0, "fval": 1.0})}
    base, one, many = io.StringIO(), io.StringIO(), io.StringIO()
    driver.run(dict(fake), stream=base)
    r1 = driver.run(dict(fake), stream=one, certified="solve", certify=False)
    assert one.getvalue().splitlines()[3].split("|")[1].strip() == "Fake"
    cells = lambda text: [c.strip() for c in text.getvalue().splitlines()[3].split("|")]
    assert cells(one) == cells(base)
    assert list(r1["log_dicts"]) == ["Fake", "Certified"]
    assert len(one.getvalue().splitlines()) == len(base.getvalue().splitlines()) + 1
    assert float(r1["log_dicts"]["Certified"]["optval"]) > 0
    r2 = driver.run(dict(fake), stream=many, certified="path", size=(40, 130, 3), seed=SEED)
    assert len(r2["log_dicts"]) == 11 and list(r2["log_dicts"])[1].startswith("Certified mu=")
    assert int(r2["log_dicts"][list(r2["log_dicts"])[1]]["iter"]) == 0
