"""Sample weights and cross-validation on the GPU (DESIGN.md "Sample weights and cross-validation").
Reference: tests/sw_ref.py, which reduces every weighted problem to the existing references on
(sqrt(w) o A, sqrt(w) o b); the library never forms that pair.

1. The weighted finalize (glx.kernels.cert_fin_sw). r^ = fl(sum of the slabs in slab order) - b and
   r_w = fl(w r^) are one rounded operation each on values the test holds exactly, so they are compared
   bit for bit with NumPy in the dtype. Each of the three sums adds m l terms that carry two roundings
   in double ((w r^) r^; for float32 inputs the first product is exact), and m l - 1 additions:
   gamma_{ml+3}(eps64) sum |terms| against longdouble on the same r^. The bar is a function of m l, so
   it holds as it stands at (2050, 128) and (262147, 1), where the grid of 1024 workgroups is full and
   256 and 3 threads take a second element (two trips, the second ragged; S = 0, 1, 3, with and
   without hold-out weights, and the unweighted kernel on the same inputs).
2. The weighted column norms (glx.kernels.col_norms_sw): test_gpu_screen's bar with one more
   rounding per term ((w a) a): (m + 3) eps64 / 2 relative (+ eps32 / 2 for float32 inputs, whose
   reference is longdouble on the float64 values they were rounded from; the weights are given in the
   dtype and are exact). (3, 262214) and (130, 262214) are past the cap of 1024 column blocks: 70
   lanes walk a second column, in one slab and in three.
3. Certificates. Ones against None bit for bit. Random weights against sw_ref in longdouble with
   test_gpu_certificate's bars, the weights carried through them: dr is the product's elementwise bar,
   d(w r) = w dr + eps / 2 |w r|, dg = (m + 2) eps |A|^T |w r| + |A|^T d(w r).
4. Solves. P* <= P_w(x) <= P* + gap+ and 1/2 ||A~ (x - x*)||^2 <= P_w(x) - P* <= gap+, where gap+ is the
   rounding guard's upper bound of the true gap from the solve's own record (sw_ref.guard, checked
   against the native guard on the CPU): "the gap plus the rounding bar" in its rigorous form. Two
   solutions of one problem are therefore within sqrt(2 gap+_1) + sqrt(2 gap+_2) in the A~ seminorm and
   their objectives, evaluated in longdouble, within gap+_1 + gap+_2.
5. holdout_loss against longdouble NumPy on the returned x: gamma_{ml+3}(eps64) of the sum plus the
   product's bar dr_jc = gamma_{n+2}(eps) ||a_j|| ||x_c|| carried through v (2 |r| dr + dr^2).
6. Cross-validation on the issue's instance: the indices of the reference curve (re-derived on the CPU
   in test_sample_weight_cpu.test_cv_reference_indices: best 5, one_se 4, at 1e-6 and 1e-8).
"""
import functools
import io

import numpy as np
import pytest

import certificate_ref as cref
import group_ref as gr
import screen_ref as sr
import sw_ref as sw

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS64 = sr.EPS64
SEED = sw.SEED


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(a, dtype=None):
    torch = _torch()
    a = np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a).astype(dtype)
    return torch.as_tensor(a, device="cuda")


def _eps(dt):
    return float(np.finfo(dt).eps)


# ------------------------------------------------------------------------------------------ 1
def _fin_weights(g, m, dt):
    w = g.uniform(0.0, 3.0, m).astype(dt)
    w[::4] = 0
    if m > 1:
        w[1] = np.finfo(dt).tiny / 4          # a subnormal weight
    v = g.uniform(0.0, 2.0, m).astype(dt)
    v[1::3] = 0
    return w, v


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("S", [0, 1, 3])
# (2050 x 128 and 262147 x 1: past the 1024-workgroup cap of 262144 elements, so the first 256 and the
# first 3 threads take a second element; the row of an element comes from idx / l at both l)
@pytest.mark.parametrize("shape", [(5, 3), (64, 16), (67, 1), (130, 128), (2050, 128), (262147, 1)],
                         ids=lambda s: "%dx%d" % s)
def test_weighted_finalize(shape, S, dt):
    from glx import kernels
    m, l = shape
    g = np.random.default_rng(1000 * m + 10 * l + S)
    b = g.standard_normal((m, l)).astype(dt)
    P = g.standard_normal((S, m, l)).astype(dt) if S else None
    w, v = _fin_weights(g, m, dt)
    ax = np.zeros((m, l), dtype=dt)
    if S:
        ax = P[0].copy()
        for k in range(1, S):
            ax = (ax + P[k]).astype(dt)
    r = (ax - b).astype(dt)
    with np.errstate(under="ignore"):
        rw = (w[:, None] * r).astype(dt)
    out = kernels.cert_fin_sw(None if P is None else _dev(P), _dev(b), _dev(w), _dev(v))
    got_r, got_rw, sums = out["r"].cpu().numpy(), out["rw"].cpu().numpy(), out["sums"].cpu().numpy()
    assert np.array_equal(got_r, r) and np.array_equal(got_rw, rw)
    rl, bl = r.astype(LD), b.astype(LD)
    terms = [w.astype(LD)[:, None] * rl * rl, w.astype(LD)[:, None] * rl * bl, v.astype(LD)[:, None] * rl * rl]
    gam = sr.gamma(m * l + 3, EPS64)
    for i, t in enumerate(terms):
        err, bar = abs(float(LD(sums[i]) - np.sum(t))), gam * float(np.sum(np.abs(t)))
        print("finalize %s S=%d %s sum %d: err %.3e bar %.3e" % (shape, S, dt.__name__, i, err, bar))
        assert err <= bar, (i, err, bar)
    again = kernels.cert_fin_sw(None if P is None else _dev(P), _dev(b), _dev(w), _dev(v))
    for key in ("r", "rw", "sums"):
        assert np.array_equal(again[key].cpu().numpy(), out[key].cpu().numpy()), key
    # without hold-out weights: the same two sums, the third slot untouched; r not asked for
    two = kernels.cert_fin_sw(None if P is None else _dev(P), _dev(b), _dev(w), None, want_r=False)
    s2 = two["sums"].cpu().numpy()
    assert two["r"] is None and np.array_equal(s2[:2], sums[:2]) and np.isnan(s2[2])
    assert np.array_equal(two["rw"].cpu().numpy(), rw)
    # all-ones weights: the unweighted kernel's bits
    one = kernels.cert_fin_sw(None if P is None else _dev(P), _dev(b), _dev(np.ones(m, dtype=dt)), None)
    base = kernels.cert_fin_sw(None if P is None else _dev(P), _dev(b), None)
    assert np.array_equal(one["rw"].cpu().numpy(), base["rw"].cpu().numpy())
    assert np.array_equal(one["r"].cpu().numpy(), base["rw"].cpu().numpy())
    assert np.array_equal(one["sums"].cpu().numpy()[:2], base["sums"].cpu().numpy()[:2])


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
# (m x 262214: 70 columns past the 1024-workgroup cap, a second column for the first 70 lanes of
# workgroup 0, in one slab and in three)
@pytest.mark.parametrize("shape", [(1, 1), (63, 65), (130, 300), (4097, 70), (3, 262214), (130, 262214)],
                         ids=lambda s: "%dx%d" % s)
def test_weighted_col_norms(shape, dt):
    from glx import kernels
    m, n = shape
    g = np.random.default_rng(31 * m + n)
    A64 = g.standard_normal((m, n))
    w = g.uniform(0.0, 3.0, m).astype(dt)
    if m > 1:
        w[::3] = 0
    zero_col = n // 2
    A64[w != 0, zero_col] = 0.0               # a column that lives on zero-weight rows only
    if m == 1:
        w[:] = 0 if n == 1 else w
    want = sw.col_norms(A64, w)
    Ad = _dev(A64, dt)
    norms, stats = kernels.col_norms_sw(Ad, _dev(w))
    got, st = norms.cpu().numpy(), stats.cpu().numpy()
    bar = ((m + 3) * EPS64 / 2 + (sr.EPS32 / 2 if dt == np.float32 else 0.0)) * want
    err = np.abs(got.astype(LD) - want)
    assert np.all(err <= bar), (m, n, float(np.max(err / np.maximum(bar, 1e-300))))
    assert got[zero_col] == 0.0 and not np.signbit(got[zero_col])
    assert st[0] == got.max()
    sq = float(np.sum(got.astype(LD) ** 2))
    assert abs(st[1] - sq) <= (m + n + 2) * EPS64 * sq
    norms2, stats2 = kernels.col_norms_sw(Ad, _dev(w))
    assert np.array_equal(norms2.cpu().numpy(), got) and np.array_equal(stats2.cpu().numpy(), st)
    ones, so = kernels.col_norms_sw(Ad, _dev(np.ones(m, dtype=dt)))
    base, sb = kernels.col_norms(Ad)
    assert np.array_equal(ones.cpu().numpy(), base.cpu().numpy()) and np.array_equal(so.cpu().numpy(), sb.cpu().numpy())


def test_weighted_col_norms_nan_weight_reaches_the_maximum():
    from glx import kernels
    A = np.ones((5, 70))
    w = np.ones(5)
    w[3] = np.nan
    norms, stats = kernels.col_norms_sw(_dev(A), _dev(w))
    assert np.all(np.isnan(norms.cpu().numpy())) and np.isnan(stats.cpu().numpy()[0])


# ------------------------------------------------------------------------------------------ 3
CERT_SHAPES = [(96, 512, 16), (40, 130, 3)]


def _groups_for(n, seed=5):
    ptr = gr.draw_groups(np.random.default_rng(seed), n, sw.GROUP_SIZES)
    return ptr, np.sqrt(np.diff(ptr).astype(np.float64))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", CERT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_ones_are_bit_identical_to_none(shape, dt):
    import glx
    m, n, l = shape
    A, b, _, _ = cref.instance(SEED, m, n, l)
    A, b = A.astype(dt), b.astype(dt)
    x = (np.random.default_rng(2).standard_normal((n, l)) * (np.random.default_rng(3).random((n, 1)) < 0.3)).astype(dt)
    ones = np.ones(m)
    mu = 0.3 * glx.mu_max(A, b)
    assert glx.mu_max(A, b, sample_weight=ones) == glx.mu_max(A, b)
    fused_seen = set()
    for fused in (0, 1, 2):
        c0 = glx.certificate(x, A, b, mu, fused=fused, row_norms=True)
        c1 = glx.certificate(x, A, b, mu, fused=fused, row_norms=True, sample_weight=ones)
        fused_seen.add(c0["fused"])
        for key in ("primal", "dual", "gap", "rel_gap", "scale", "gmax", "kkt_max", "kkt_fro", "nonzero_rows", "fused"):
            assert c0[key] == c1[key], (fused, key)
        assert np.array_equal(c0["row_norms"], c1["row_norms"])
        assert "k_cert_fin_w" in c1["plan"] and "k_cert_fin_w" not in c0["plan"]
    print("ones %s %s: fused forms seen %s" % (shape, dt.__name__, sorted(fused_seen)))
    ptr, gw = _groups_for(n)
    g0 = glx.certificate(x, A, b, mu, groups=ptr, weights=gw, row_norms=True)
    g1 = glx.certificate(x, A, b, mu, groups=ptr, weights=gw, row_norms=True, sample_weight=ones)
    for key in ("primal", "dual", "gap", "rel_gap", "scale", "gmax", "kkt_max", "kkt_fro", "nonzero_groups"):
        assert g0[key] == g1[key], key
    assert np.array_equal(g0["group_norms"], g1["group_norms"])
    assert glx.mu_max(A, b, ptr, gw, sample_weight=ones) == glx.mu_max(A, b, ptr, gw)


def test_ones_record_and_g_out_are_bit_identical():
    """All eight record values, G_out and the row norms through the C entries themselves."""
    import ctypes
    from glx import _lib
    torch = _torch()
    for (m, n, l) in CERT_SHAPES:
        for tdt, gdt in ((torch.float64, _lib.GLX_F64), (torch.float32, _lib.GLX_F32)):
            A, b, _, _ = cref.instance(SEED, m, n, l)
            Ad, bd = _dev(A).to(tdt), _dev(b).to(tdt)
            xd = _dev(np.random.default_rng(4).standard_normal((n, l))).to(tdt)
            ones = torch.ones(m, dtype=tdt, device="cuda")
            nb = ctypes.c_size_t(0)
            _lib.check(_lib.lib().glx_certificate_sw_workspace_bytes(gdt, m, n, l, ctypes.byref(nb)))
            ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
            res = []
            for sw_ptr in (None, ones.data_ptr()):
                rec, hs = (ctypes.c_double * 8)(), ctypes.c_double(-1.0)
                G = torch.full((n, l), float("nan"), dtype=tdt, device="cuda")
                rn = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                _lib.check(_lib.lib().glx_certificate_sw(gdt, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), 0.5,
                                                         0, sw_ptr, None, G.data_ptr(), rn.data_ptr(), rec,
                                                         ctypes.byref(hs), ws.data_ptr(), ws.numel(), None))
                torch.cuda.synchronize()
                res.append((list(rec), G.cpu().numpy(), rn.cpu().numpy(), hs.value))
            assert res[0][0] == res[1][0] and res[0][3] == res[1][3] == 0.0
            assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
            # and the unweighted entry itself
            rec = (ctypes.c_double * 8)()
            _lib.check(_lib.lib().glx_certificate(gdt, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), 0.5, 0,
                                                  None, None, rec, ws.data_ptr(), ws.numel(), None))
            assert list(rec) == res[0][0]


def _wcert_bars(x, A, b, mu, w, dt, zero_x=False):
    """test_gpu_certificate._cert_bars with the weights carried through (docstring, 3)."""
    import test_gpu_certificate as tc
    W = tc._wide(dt)
    eps = _eps(dt)
    m, n = A.shape
    muT = float(dt(mu))
    ref = sw.certificate(x, A, b, muT, w, wide=W)
    A64, x64, b64 = (np.abs(a.astype(np.float64)) for a in (A, x, b))
    w64 = w.astype(np.float64)[:, None]
    r_true = np.abs((A.astype(W) @ x.astype(W) - b.astype(W)).astype(np.float64))
    dr = np.zeros(b.shape) if zero_x else (n + 2) * eps * (A64 @ x64 + b64)
    drw = w64 * dr + eps / 2 * w64 * r_true
    dg = (m + 2) * eps * (A64.T @ (w64 * r_true)) + A64.T @ drw
    g_T = ref["g"].astype(dt)
    _, bars = tc._row_bars(x, g_T, muT, dt, dg=dg + eps / 2 * np.abs(ref["g"].astype(np.float64)))
    rr, rb = float(ref["rr"]), float(ref["rb"])
    bars["rr"] = tc.C * (np.sum(w64 * (2 * r_true * dr + dr * dr)) + (tc.CSUM + 2) * EPS64 * rr)
    bars["rb"] = tc.C * (np.sum(w64 * b64 * dr) + (tc.CSUM + 2) * EPS64 * np.sum(w64 * r_true * b64))
    gmax, s, sx = float(ref["gmax"]), float(ref["scale"]), float(ref["sum_xnorm"])
    dgm = bars["gmax"] / tc.C
    ds = min(1.0, muT / max(gmax - dgm, tc.TINY)) - min(1.0, muT / (gmax + dgm)) if gmax > 0 else 0.0
    host = 4 * EPS64 * (0.5 * (1 + s * s) * rr + abs(s * rb) + muT * sx)
    bars["gap"] = tc.C * (0.5 * (1 + s * s) * bars["rr"] / tc.C + s * bars["rb"] / tc.C
                          + muT * bars["sum_xnorm"] / tc.C + abs(s * rr + rb) * ds + host)
    return ref, bars


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", CERT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_certificate_with_random_weights(shape, dt):
    import glx
    m, n, l = shape
    A, b, _, _ = cref.instance(SEED, m, n, l)
    A, b = A.astype(dt), b.astype(dt)
    w = sw.draw_weights(sw.WSEED, m).astype(dt)
    assert (w == 0).sum() == m // 4
    W = np.longdouble if dt == np.float64 else np.float64
    # mu_max and the certificate at x = 0
    want = float(sw.mu_max(A, b, w, wide=W))
    mm = glx.mu_max(A, b, sample_weight=w)
    zero = np.zeros((n, l), dtype=dt)
    _, bars0 = _wcert_bars(zero, A, b, want, w, dt, zero_x=True)
    print("mu_max %s %s: got %.17g ref %.17g bar %.3e" % (shape, dt.__name__, mm, want, bars0["gmax"]))
    assert abs(mm - want) <= bars0["gmax"]
    c0 = glx.certificate(zero, A, b, mm, sample_weight=w)
    _, bars0 = _wcert_bars(zero, A, b, mm, w, dt, zero_x=True)
    assert c0["scale"] == 1.0 and c0["kkt_max"] == 0.0 and c0["nonzero_rows"] == 0 and abs(c0["gap"]) <= bars0["gap"]
    # a random sparse point
    g = np.random.default_rng(12)
    x = (g.standard_normal((n, l)) * (g.random((n, 1)) < 0.2) * 0.05).astype(dt)
    mu = float(dt(0.3 * want))
    ref, bars = _wcert_bars(x, A, b, mu, w, dt)
    c = glx.certificate(x, A, b, mu, sample_weight=w, row_norms=True)
    got = {"gmax": c["gmax"], "kkt_max": c["kkt_max"], "gap": c["gap"]}
    for key in ("gmax", "kkt_max", "gap"):
        err = abs(float(got[key]) - float(ref[key]))
        print("weighted certificate %s %s %s: err %.3e bar %.3e" % (shape, dt.__name__, key, err, bars[key]))
        assert err <= bars[key], (key, err, bars[key])
    perr = abs(c["primal"] - float(ref["primal"]))
    assert perr <= 0.5 * bars["rr"] + mu * bars["sum_xnorm"] + 4 * EPS64 * abs(float(ref["primal"]))
    assert np.all(np.abs(c["row_norms"] - ref["row_norms"].astype(np.float64)) <= bars["gnorm"])
    assert c["nonzero_rows"] == ref["nonzero_rows"]
    # groups on top: the record's loss terms are the row certificate's bits (the same finalize),
    # mu_max equals the reference's within the group norm's bar
    ptr, gw = _groups_for(n)
    cg = glx.certificate(x, A, b, mu, groups=ptr, weights=gw, sample_weight=w)
    refg = sw.certificate(x, A, b, mu, w, ptr, gw, wide=W)
    K = int(np.diff(ptr).max()) * l
    gK = sr.gamma(K + 3, _eps(dt))
    dgq = np.sqrt(np.add.reduceat(bars["gnorm"] ** 2, ptr[:-1].astype(np.intp))) / gw
    bar_g = float(np.max(dgq)) + 2 * gK * float(refg["gmax"])
    assert abs(cg["gmax"] - float(refg["gmax"])) <= bar_g, (cg["gmax"], float(refg["gmax"]), bar_g)
    bar_sx = 2 * (gK + 32 * EPS64) * float(refg["sum_xnorm"])
    assert abs(cg["primal"] - float(refg["primal"])) <= 0.5 * bars["rr"] + mu * bar_sx + 4 * EPS64 * float(refg["primal"])
    assert cg["nonzero_groups"] == refg["nonzero_groups"]
    mmg = glx.mu_max(A, b, ptr, gw, sample_weight=w)
    wantg = float(sw.mu_max(A, b, w, ptr, gw, wide=W))
    g0 = np.abs(A.astype(np.float64)).T @ (w.astype(np.float64)[:, None] * np.abs(b.astype(np.float64)))
    dg0 = (m + 3) * _eps(dt) * g0
    bar0 = float(np.max(np.sqrt(np.add.reduceat(np.sum(dg0 * dg0, axis=1), ptr[:-1].astype(np.intp))) / gw)) \
        + 2 * gK * wantg
    assert abs(mmg - wantg) <= bar0, (mmg, wantg, bar0)


# ------------------------------------------------------------------------------------------ 4
SOLVE_CASES = [(96, 512, 16, 0.5), (96, 512, 16, 0.1), (40, 130, 3, 0.5), (40, 130, 3, 0.1)]
TOL = 1e-10


def _figures(A, b, w):
    cn = np.asarray(sw.col_norms(A, w), dtype=np.float64)
    return float(cn.max()), float(np.sum(cn * cn)), float(np.sqrt(np.sum(w[:, None] * b * b)))


def _gap_plus(x, A, b, mu, w=None, eps=EPS64):
    """gap+ of the rounding guard from the GPU's own record of x (docstring, 4)."""
    from glx.certificate import record
    m, n = A.shape
    l = b.shape[1]
    if w is None:
        rec = record(x, A, b, mu)
        return sr.guard(rec, mu, eps, m, n, l, *_figures(A, b, np.ones(m)))[1]
    return sw.guard(_record_sw(x, A, b, mu, w), mu, eps, m, n, l, *_figures(A, b, w))[1]


def _record_sw(x, A, b, mu, w, gw=None):
    from glx.certificate import _inputs, _record_sw as rec_sw, _group_record_sw, _sw_device
    xd, Ad, bd = _inputs(x, A, b)
    swd = _sw_device(np.ascontiguousarray(w, dtype=A.dtype), Ad.device)
    if gw is not None:
        return _group_record_sw(xd, Ad, bd, mu, gw, False, swd)[0]
    return rec_sw(xd, Ad, bd, mu, 0, False, swd)[0]


@functools.lru_cache(maxsize=None)
def _solved(m, n, l, ratio, kind, screen=True, f32=False, tol=TOL):
    import glx
    ref = sw.reference_solution(m, n, l, ratio, kind, f32)
    dt = np.float32 if f32 else np.float64
    return glx.solve_certified(ref["A"].astype(dt), ref["b"].astype(dt), ref["mu"], tol=tol, screen=screen,
                               sample_weight=ref["w"])


def _seminorm(A, w, d):
    """||sqrt(w) o (A d)||_F in longdouble."""
    r = A.astype(LD) @ d.astype(LD)
    return float(np.sqrt(np.sum(w.astype(LD)[:, None] * r * r)))


@pytest.mark.parametrize("case", SOLVE_CASES, ids=lambda c: "%dx%dx%d@%g" % c)
def test_ones_solve(case):
    import glx
    m, n, l, ratio = case
    A, b, _, _ = cref.instance(SEED, m, n, l)
    mu = ratio * glx.mu_max(A, b)
    ones = np.ones(m)
    x0, i0 = glx.solve_certified(A, b, mu, tol=TOL, screen=False)
    x1, i1 = glx.solve_certified(A, b, mu, tol=TOL, screen=False, sample_weight=ones)
    assert np.array_equal(x0, x1) and i0["iterations"] == i1["iterations"] and i0["step"] == i1["step"]
    assert i0["primal"] == i1["primal"] and i0["gap"] == i1["gap"] and i1["converged"]
    xs, isc = glx.solve_certified(A, b, mu, tol=TOL, screen=True, sample_weight=ones)
    xn, inn = glx.solve_certified(A, b, mu, tol=TOL, screen=True)
    assert isc["converged"] and inn["converged"]
    dp = float(abs(sw.primal(xs, A, b, mu, ones) - sw.primal(xn, A, b, mu, ones)))      # (in longdouble)
    g1, g2 = _gap_plus(xs, A, b, mu, ones), _gap_plus(xn, A, b, mu)
    print("ones %s: |P1 - P2| %.3e, gap+ %.3e %.3e, kept %d / %d" % (case, dp, g1, g2, isc["kept"], inn["kept"]))
    assert dp <= g1 + g2


@pytest.mark.parametrize("kind", ["mask", "int"])
@pytest.mark.parametrize("case", SOLVE_CASES, ids=lambda c: "%dx%dx%d@%g" % c)
def test_mask_and_integer_weights_solve_the_row_problems(case, kind):
    """A 0/1 mask against solve_certified(A[mask], b[mask]); integer weights against the problem with
    rows repeated."""
    import glx
    m, n, l, ratio = case
    ref = sw.reference_solution(m, n, l, ratio, kind)
    A, b, w, mu = ref["A"].copy(), ref["b"].copy(), ref["w"].copy(), ref["mu"]
    x1, i1 = _solved(m, n, l, ratio, kind)
    rows = np.repeat(np.arange(m), w.astype(np.int64))
    A2, b2 = np.ascontiguousarray(A[rows]), np.ascontiguousarray(b[rows])
    x2, i2 = glx.solve_certified(A2, b2, mu, tol=TOL)
    assert i1["converged"] and i2["converged"]
    g1, g2 = _gap_plus(x1, A, b, mu, w), _gap_plus(x2, A2, b2, mu)
    dist = _seminorm(A, w, x1 - x2)
    bound = np.sqrt(2 * g1) + np.sqrt(2 * g2)
    P1, P2 = sw.primal(x1, A, b, mu, w), sw.primal(x2, A, b, mu, w)
    p1, dp = float(P1), float(abs(P1 - P2))                                              # (in longdouble)
    print("%s %s: ||A~ (x1 - x2)|| %.3e bound %.3e; |P1 - P2| %.3e bound %.3e (reported gaps %.3e %.3e)"
          % (kind, case, dist, bound, dp, g1 + g2, i1["gap"], i2["gap"]))
    assert dist <= bound
    assert dp <= g1 + g2
    assert g1 <= 10 * TOL * p1 and g2 <= 10 * TOL * p1          # the bounds are of the tolerance's size, not vacuous


@pytest.mark.parametrize("case", SOLVE_CASES, ids=lambda c: "%dx%dx%d@%g" % c)
def test_general_weights_solve(case):
    m, n, l, ratio = case
    ref = sw.reference_solution(m, n, l, ratio, "general")
    A, b, w, mu = ref["A"].copy(), ref["b"].copy(), ref["w"].copy(), ref["mu"]
    x, info = _solved(m, n, l, ratio, "general")
    assert info["converged"] and info["rel_gap"] <= TOL
    gp = _gap_plus(x, A, b, mu, w)
    excess = float(sw.primal(x, A, b, mu, w) - sw.primal(ref["x"], A, b, mu, w))
    print("general %s: P(x) - P(x*) %.3e, reported gap %.3e, gap+ %.3e, %d iterations, compactions %s, kept %d"
          % (case, excess, info["gap"], gp, info["iterations"], info["kept_history"], info["kept"]))
    assert excess <= gp and gp <= info["gap"] + 10 * TOL * info["primal"]
    assert excess >= -float(ref["gap"]) - 4 * EPS64 * info["primal"]
    support = np.nonzero(np.sqrt(np.sum(ref["x"] ** 2, axis=1)) != 0)[0]
    assert set(support) <= set(info["kept_rows"].tolist())
    screened = np.ones(n, dtype=bool)
    screened[info["kept_rows"]] = False
    assert not np.any(screened & ~(ref["gtheta"] < LD(mu)))
    if ratio == 0.5:
        assert info["compactions"] >= 1 and info["width"] < n
    assert "k_cert_fin_w" in info["plan"]


def test_general_weights_grouped_solve():
    import glx
    m, n, l, ratio = 96, 512, 16, 0.5
    ref = sw.group_reference_solution(m, n, l, ratio)
    A, b, w, ptr, gw, mu = (ref[k].copy() if hasattr(ref[k], "copy") else ref[k] for k in ("A", "b", "w", "ptr", "gw", "mu"))
    x, info = glx.solve_certified(A, b, mu, tol=TOL, groups=ptr, weights=gw, sample_weight=w)
    assert info["converged"] and info["compactions"] >= 1
    At, _ = sw.reduce(A, b, w)
    gcn = np.asarray(gr.group_cnorms(At, ptr, gw), dtype=np.float64)
    rec = _record_sw(x, A, b, mu, w, (np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(gw)))
    gp = sw.group_guard(rec, mu, EPS64, m, n, l, int(np.diff(ptr).max()), float(gw.min()), float(gcn.max()),
                        float(np.sum(At * At)), float(np.sqrt(np.sum(w[:, None] * b * b))))[1]
    excess = float(sw.primal(x, A, b, mu, w, ptr, gw) - sw.primal(ref["x"], A, b, mu, w, ptr, gw))
    print("grouped: P(x) - P(x*) %.3e gap+ %.3e reported %.3e, kept %d groups" % (excess, gp, info["gap"], info["kept"]))
    assert excess <= gp
    active = np.nonzero(gr.group_norms(ref["x"], ptr) != 0)[0]
    assert set(active) <= set(info["kept_groups"].tolist())


def test_general_weights_solve_f32():
    m, n, l, ratio = 96, 512, 16, 0.5
    ref = sw.reference_solution(m, n, l, ratio, "general", True)
    x, info = _solved(m, n, l, ratio, "general", True, True, 1e-4)
    print("f32: %d iterations, compactions %s, kept %d, rel_gap %.2e"
          % (info["iterations"], info["kept_history"], info["kept"], info["rel_gap"]))
    assert x.dtype == np.float32 and info["converged"]
    screened = np.ones(n, dtype=bool)
    screened[info["kept_rows"]] = False
    assert not np.any(screened & ~(ref["gtheta"] < LD(ref["mu"])))
    assert not np.any(screened & (np.sqrt(np.sum(ref["x"] ** 2, axis=1)) != 0))


def test_path_with_weights():
    import glx
    m, n, l = 96, 512, 16
    A, b, _, _ = cref.instance(SEED, m, n, l)
    w = sw.weights_of("general", m)
    tol = 1e-6
    out = glx.path(A, b, n_mus=4, mu_min_ratio=0.05, tol=tol, sample_weight=w)
    mus = [o[0] for o in out]
    assert mus[0] == glx.mu_max(A, b, sample_weight=w) and len(out) == 4
    mu0, x0, i0 = out[0]
    assert np.all(x0 == 0) and i0["iterations"] == 0 and i0["gap"] == 0.0 and i0["converged"]
    for mu, x, info in out:
        assert info["converged"] and info["rel_gap"] <= tol and info["mu"] == mu
    warm = sum(o[2]["iterations"] for o in out)
    cold = sum(glx.solve_certified(A, b, mu, tol=tol, sample_weight=w)[1]["iterations"] for mu in mus)
    print("weighted path: warm-started %d iterations, cold %d" % (warm, cold))
    assert warm < cold


# ------------------------------------------------------------------------------------------ 5
def _holdout_bar(x, A, b, v, eps):
    m, n = A.shape
    l = b.shape[1]
    r = np.abs(A.astype(LD) @ x.astype(LD) - b.astype(LD)).astype(np.float64)
    an = np.sqrt(np.sum(A.astype(np.float64) ** 2, axis=1))[:, None]
    xn = np.sqrt(np.sum(x.astype(np.float64) ** 2, axis=0))[None, :]
    dr = sr.gamma(n + 2, eps) * an * xn
    vv = v.astype(np.float64)[:, None]
    total = float(np.sum(vv * r * r))
    bar_sum = float(np.sum(vv * (2 * r * dr + dr * dr))) + sr.gamma(m * l + 3, EPS64) * total
    return 0.5 * bar_sum / float(np.sum(v)) + 4 * EPS64 * 0.5 * total / float(np.sum(v))


def test_holdout_loss():
    import glx
    m, n, l = 40, 130, 3
    A, b, _, _ = cref.instance(SEED, m, n, l)
    lab = np.arange(m) % 4
    tr, ho = (lab != 1).astype(np.float64) * 1.5, (lab == 1).astype(np.float64) * 0.5
    mu = 0.1 * glx.mu_max(A, b, sample_weight=tr)
    x, info = glx.solve_certified(A, b, mu, tol=1e-8, sample_weight=tr, holdout_weight=ho)
    want = float(sw.holdout_loss(x, A, b, ho))
    bar = _holdout_bar(x, A, b, ho, EPS64)
    print("holdout_loss: got %.17g ref %.17g err %.3e bar %.3e" % (info["holdout_loss"], want,
                                                                   abs(info["holdout_loss"] - want), bar))
    assert info["converged"] and abs(info["holdout_loss"] - want) <= bar
    assert info["holdout_loss"] == 0.5 * info["holdout_sum"] / float(np.sum(ho))
    # hold-out weights alone: held out of the unweighted fit (sample weights of ones)
    x2, i2 = glx.solve_certified(A, b, mu, tol=1e-8, holdout_weight=ho)
    x3, i3 = glx.solve_certified(A, b, mu, tol=1e-8, sample_weight=np.ones(m), holdout_weight=ho)
    assert np.array_equal(x2, x3) and i2["holdout_loss"] == i3["holdout_loss"]
    # the path carries it on every entry
    for mu_, x_, i_ in glx.path(A, b, n_mus=3, mu_min_ratio=0.1, tol=1e-6, sample_weight=tr, holdout_weight=ho):
        assert abs(i_["holdout_loss"] - float(sw.holdout_loss(x_, A, b, ho))) <= _holdout_bar(x_, A, b, ho, EPS64)


# ------------------------------------------------------------------------------------------ 6
@functools.lru_cache(maxsize=None)
def _cv(label_array=False, refit=False):
    import glx
    A, b = sw.cv_instance()
    folds = np.arange(A.shape[0]) % 5 if label_array else 5
    return glx.cv_path(A, b, folds=folds, n_mus=10, mu_min_ratio=1e-2, tol=1e-6, refit=refit)


def test_cv_path():
    import glx
    from glx.cv import aggregate
    A, b = sw.cv_instance()
    cv = _cv(False, True)
    assert cv["folds"] == 5 and cv["fold_loss"].shape == (5, 10) and len(cv["mus"]) == 10
    assert cv["mus"][0] == glx.mu_max(A, b)
    print("cv mean %s\ncv se %s\nbest %d one_se %d" % (np.round(cv["mean"], 4), np.round(cv["se"], 4), cv["best"],
                                                       cv["one_se"]))
    assert cv["best"] == 5 and cv["one_se"] == 4
    assert cv["mu_best"] == cv["mus"][5] and cv["mu_one_se"] == cv["mus"][4]
    agg = aggregate(cv["fold_loss"], cv["mus"])
    assert np.array_equal(agg["mean"], cv["mean"]) and np.array_equal(agg["se"], cv["se"])
    mean, se, best, one = sw.cv_aggregate(cv["fold_loss"])
    assert np.allclose(mean, cv["mean"], rtol=8 * EPS64, atol=0) and np.allclose(se, cv["se"], rtol=64 * EPS64, atol=0)
    assert (best, one) == (5, 4)
    lab = np.arange(120) % 5
    for k in range(5):
        assert len(cv["info"][k]) == 10 and all(i["converged"] for i in cv["info"][k])
    # every fold_loss is the NumPy loss of the GPU's own x: cv_path keeps no x, so each fold's path is
    # solved again here, which gives the same bits (the folds share A, b and the grid)
    for k in range(5):
        tr, ho = sw.fold_vectors(lab, k)
        out = glx.path(A, b, mus=cv["mus"], tol=1e-6, sample_weight=tr, holdout_weight=ho)
        for i, (mu, x, info) in enumerate(out):
            assert info["holdout_loss"] == cv["fold_loss"][k, i]            # the folds share A, b: the same bits
            assert abs(info["holdout_loss"] - float(sw.holdout_loss(x, A, b, ho))) <= _holdout_bar(x, A, b, ho, EPS64)
    mu_r, x_r, info_r = cv["refit"]
    assert mu_r == cv["mu_best"] and info_r["converged"] and info_r["rel_gap"] <= 1e-6 and x_r.shape == (256, 4)


def test_cv_path_label_array_gives_the_same_bits():
    a, c = _cv(False, True), _cv(True, False)
    assert np.array_equal(a["fold_loss"], c["fold_loss"]) and np.array_equal(a["mean"], c["mean"])
    assert np.array_equal(a["se"], c["se"]) and (a["best"], a["one_se"]) == (c["best"], c["one_se"])
    assert "refit" not in c


# ------------------------------------------------------------------------------------------ driver
def test_driver_cv_table():
    """python -m glx.driver --cv 3: the Statistics table is what it is without the flag, and the CV
    table follows it with one line per mu and exactly one best marker."""
    from glx import driver
    fake = {"Fake": lambda x0, A, b, mu, opts: (np.zeros_like(x0), 3, {"tt": 0.0, "fval": 1.0})}
    base, with_cv = io.StringIO(), io.StringIO()
    driver.run(dict(fake), stream=base, size=(40, 130, 3), seed=SEED)
    res = driver.run(dict(fake), stream=with_cv, size=(40, 130, 3), seed=SEED, cv=3)
    lines = with_cv.getvalue().splitlines()
    nbase = len(base.getvalue().splitlines())
    assert lines[:nbase] == base.getvalue().splitlines()
    tail = lines[nbase:]
    assert tail[0].startswith("# Cross-validation (3 folds)")
    rows = tail[2:]
    assert len(rows) == 10 == len(res["cv"]["mus"])
    assert sum("best" in r for r in rows) == 1 and sum("1-SE" in r for r in rows) == 1
    assert "best" in rows[res["cv"]["best"]] and "1-SE" in rows[res["cv"]["one_se"]]
