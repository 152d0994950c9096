"""The sparse-group lasso on the GPU: the five kernels of kernels_sgl.hip one launch at a time, then the
certificate, the certified solve, the path, sample weights and the refusals. Reference: tests/sgl_ref.py.
u = eps / 2 is the unit roundoff of the working dtype T, u64 that of float64, l the columns, R the rows of a
group and k = R l its elements. Every bar is first order in u times (1 + 4 e), e the largest relative error
it composes.

1. sgl_step (k_sgl_fista) against sgl_ref.step_ref, longdouble on the same T inputs: test_gpu_group.py's bars
   for k_group_fista with one more level. Every row's rho_i = ||w_i|| is placed at t a (1 +- d_i), d_i in
   [0.06, 0.49], by scaling its y and g, and every group's q_g at t c_g (1 +- e_g) by choosing its weight, so
   nothing flips side and the two cancellations are bounded by 1 / d and 1 / e:
     w_e = y_e - t g_e                 |dw_e| <= a_e = u (2 |t g_e| + |w_e|)
     rho = sqrt(sum w_e^2)             e_rho = (l / 2 + 1) u + ||a||_2 / rho
     c1 = rho - t a                    e_c1 = ((1 + d) e_rho + u) / d + u
     q = sqrt(sum c1_i^2)              e_q = max_i e_c1 + (R / 2 + 1) u
     c2 = q - t c_g                    e_c2 = ((1 + e) e_q + 2 u) / e + u       (t c_g is two roundings)
     xc_e = ((w_e c1) / rho) c2 / q    |dxc_e| <= (c1 c2 / (rho q)) a_e + |xc_e| (e_c1 + e_rho + e_c2 + e_q + 4 u)
   and xc = +0 exactly in a row or a group on the other side. v_next, y_next and the sums as in
   test_gpu_group.py; the penalty sum carries tau (l / 2 + 3) u per row norm and (1 - tau) (k / 2 + 4) u per
   group norm.
2. sgl_certificate_step (k_sgl_cert) against sgl_ref.cert_terms on the kernel's own g, and sgl_dual_scale
   (k_sgl_dual_scale) against the exact s_g by sorting. A term of the KKT distance composes norms of at most
   k elements with a handful of products: (k / 2 + 8) u times the magnitudes it adds, rho_i + a + c_g for a
   row and ||rho_[g]|| + sqrt(R) a + c_g for a zero group. phi_g's relative sensitivity to s is at least 1, so
   evaluating phi_g <= c_g in float64 can accept an s at most (R + 16) u64 above the exact supremum; below it
   the kernel's termination rule allows (a + c_g) / max rho 2^-56 (sgl_ref.halving_bound).
3. sgl_screen and sgl_expand: flags and lists equal sgl_ref's on the same float64 inputs (the data keeps every
   test 1e-9 away from equality, asserted).
4. - 7. The public interface against sgl_ref.reference_solution. Two points x, x' with gaps g, g' obey
   ||A (x - x')|| <= sqrt(2 g) + sqrt(2 g') (the loss is 1-strongly convex in A x).
"""
import ctypes

import numpy as np
import pytest

import group_ref as gr
import sgl_ref as sr

pytestmark = pytest.mark.gpu

LD = sr.LD
TAUS = [0.3, 0.9, 1.0]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(a, dtype=None):
    torch = _torch()
    a = np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a).astype(dtype)
    return torch.as_tensor(a, device="cuda")


def _u(dt):
    return float(np.finfo(dt).eps) / 2


def _gsum(v, ptr):
    return np.add.reduceat(v, np.asarray(ptr[:-1], dtype=np.intp))


def _gmax(v, ptr):
    return np.maximum.reduceat(v, np.asarray(ptr[:-1], dtype=np.intp))


def _rows(v, ptr):
    return gr.expand_rows(v, ptr)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _many_groups(g, G, pool):
    return np.concatenate(([0], np.cumsum(g.choice(pool, size=G)))).astype(np.int32)


# ------------------------------------------------------------------------------------------ 1
# (n, rows, l, pool): l in {1, 3, 32, 128} (4, 4, 32 and 64 lanes per row, the last with two elements per
# lane), n no multiple of 64, runs of 64 and 65 rows, and 4101 groups: five past one trip of 1024 workgroups
STEP_CASES = [(130, 130, 3, gr.POOL_RAGGED), (475, 512, 32, gr.POOL_SMALL), (203, 256, 3, gr.POOL_LONG),
              (70, 70, 1, (1, 2)), (90, 128, 128, (1, 3, 5)), (0, 0, 1, (1, 2))]
# every lane layout of sgl_dispatch by itself, at both ends of its range of l: (4, 1) at l = 4, (16, 1) at 5 and
# 16, (32, 1) at 17, (64, 1) at 33 and 64, (64, 2) at 65 and at 127, where the second element of the last lanes
# is masked. About 130 rows in groups of up to 5: more rows than the 4, 2 or 1 sub-teams of a wave from l = 5 on.
STEP_CASES += [(129, 129, 4, gr.POOL_RAGGED), (130, 192, 5, (1, 3, 5)), (131, 131, 16, gr.POOL_RAGGED),
               (129, 129, 17, (1, 3, 5)), (130, 192, 33, gr.POOL_RAGGED), (131, 131, 64, (1, 3, 5)),
               (129, 129, 65, gr.POOL_RAGGED), (130, 192, 127, (1, 3, 5))]
T_STEP, MU_STEP = 0.3, 0.7


def _step_inputs(n, rows, l, pool, dt, tau, seed):
    g = np.random.default_rng(seed)
    if n == 0:   # the several-trip case
        ptr = _many_groups(g, 4101, pool)
        n = int(ptr[-1])
        rows = n + 63
    else:
        ptr = gr.draw_groups(g, n, pool)
    G = ptr.size - 1
    y = g.standard_normal((rows, l))
    gv = g.standard_normal((rows, l))
    xk = g.standard_normal((rows, l)) * (g.random((rows, l)) < 0.7)
    ta = T_STEP * tau * MU_STEP
    d = g.uniform(0.08, 0.45, n) * np.where(g.random(n) < 0.6, 1.0, -1.0)
    rho = sr.row_norms((y - T_STEP * gv)[:n])
    alpha = (ta * (1.0 + d) / rho)[:, None]
    y[:n] *= alpha
    gv[:n] *= alpha
    zero = int(g.integers(G))
    y[ptr[zero]:ptr[zero + 1]] = 0.0
    gv[ptr[zero]:ptr[zero + 1]] = 0.0
    y, gv, xk = y.astype(dt), gv.astype(dt), xk.astype(dt)
    # the weights put q_g at t c_g (1 +- e); a group with no row above t a keeps sqrt(size)
    wl = y[:n].astype(LD) - LD(dt(T_STEP)) * gv[:n].astype(LD)
    c1 = np.maximum(sr.row_norms(wl) - LD(dt(ta)), 0)
    q = np.sqrt(_gsum(c1 * c1, ptr)).astype(np.float64)
    e = g.uniform(0.08, 0.45, G) * np.where(g.random(G) < 0.6, 1.0, -1.0)
    tc = T_STEP * (1.0 - tau) * MU_STEP
    w = np.sqrt(np.diff(ptr).astype(np.float64))
    if tc > 0:
        w = np.where(q > 0, q / (tc * (1.0 + e)), w)
    return ptr, w.astype(dt).astype(np.float64), y, gv, xk, zero


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "%d(%d)x%d-%s" % (c[0], c[1], c[2], c[3][-1]))
def test_sgl_step(case, dt, tau):
    from glx import kernels
    torch = _torch()
    n, rows, l, pool = case
    u = _u(dt)
    ptr, w, y, gv, xk, zero = _step_inputs(n, rows, l, pool, dt, tau, 11 + n + l)
    n, rows = int(ptr[-1]), y.shape[0]
    thres = float(np.finfo(dt).tiny)
    theta, theta_next = 2.0 / 4, 2.0 / 5
    xc, vn, yn, sums, rho, q, ta, tcw = sr.step_ref(y[:n], gv[:n], xk[:n], ptr, w, T_STEP, MU_STEP, tau, thres, theta,
                                                   theta_next)
    live = np.ones(ptr.size - 1, dtype=bool)
    live[zero] = False
    lrow = _rows(live, ptr)
    dd = np.abs(rho / ta - 1)
    assert np.all(dd[lrow] >= 0.05) and np.all(dd[lrow] <= 0.5)   # the construction holds after rounding to T
    has = (q > 0) & (tcw > 0)
    ee = np.where(has, np.abs(q / np.where(tcw > 0, tcw, 1) - 1), 1)
    assert np.all(ee[has] >= 0.05) and np.all(ee[has] <= 0.5)
    # the bars of the module docstring
    R = np.diff(ptr).astype(np.float64)
    k = R * l
    tl = LD(dt(T_STEP))
    yl, gl, xl = y[:n].astype(LD), gv[:n].astype(LD), xk[:n].astype(LD)
    wv = yl - tl * gl
    a = u * (2 * np.abs(tl * gl) + np.abs(wv))
    an = np.sqrt(np.sum(a * a, axis=1))
    srho = np.where(rho > 0, rho, 1)
    e_rho = (l / 2 + 1) * u + an / srho
    on1 = rho > ta
    e_c1 = np.where(on1, ((1 + dd) * e_rho + u) / np.where(dd > 0, dd, 1) + u, 0)
    e_q = _gmax(e_c1, ptr) + (R / 2 + 1) * u
    on2 = q > tcw
    e_c2 = np.where(on2 & (tcw > 0), ((1 + ee) * e_q + 2 * u) / ee + u, np.where(on2, e_q + u, 0))
    lift = 1 + 4 * float(max(np.max(e_c1 + e_rho), np.max(e_c2 + e_q)))
    sq = np.where(q > 0, q, 1)
    f1 = np.where(on1, (rho - ta) / srho, 0)
    f2 = np.where(on2, (q - tcw) / sq, 0)
    dxc = ((f1 * _rows(f2, ptr))[:, None] * a
           + np.abs(xc) * (e_c1 + e_rho + _rows(e_c2 + e_q, ptr) + 4 * u)[:, None]) * lift
    th, a1, b1 = LD(dt(theta)), LD(dt(1.0 - theta_next)), LD(dt(theta_next))
    xo = np.where(np.abs(xl) < LD(thres), 0, xl)
    dv = ((dxc + u * np.abs(xc - xo)) / th + u * np.abs(xc - xo) / th + u * np.abs(vn)) * lift
    dy = (abs(a1) * (dxc + u * np.abs(xc)) + abs(b1) * (dv + u * np.abs(vn)) + u * np.abs(yn)) * lift
    dl = xc - yl
    u64n = n * l * gr.EPS64 / 2
    wT = w.astype(dt).astype(LD)
    xrn, xgn = sr.row_norms(xc), gr.group_norms(xc, ptr)
    drn = np.sqrt(np.sum(dxc * dxc, axis=1))
    pen_bar = (LD(tau) * np.sum(drn + ((l / 2 + 1) * u + 2 * u) * xrn)
               + LD(1 - tau) * np.sum(wT * (np.sqrt(_gsum(drn * drn, ptr)) + ((k / 2 + 1) * u + 3 * u) * xgn))) * lift
    bars = [np.sum(np.abs(gl) * (dxc + u * np.abs(dl)) + u * np.abs(gl * dl)) * lift + u64n * np.sum(np.abs(gl * dl)),
            np.sum(2 * np.abs(dl) * (dxc + u * np.abs(dl)) + u * dl * dl) * lift + u64n * np.sum(dl * dl),
            pen_bar + 2 * u64n * abs(sums[2]), np.max(dxc)]
    canary = -7.5
    names = ("xc", "v_next", "y_next")
    tdt = torch.float64 if dt == np.float64 else torch.float32
    runs = []
    for _ in range(2):
        flat = {nm: torch.full((64 + rows * l + 64,), canary, dtype=tdt, device="cuda") for nm in names}
        out = {nm: flat[nm][64: 64 + rows * l].view(rows, l) for nm in names}
        sflat = torch.full((8,), canary, dtype=torch.float64, device="cuda")
        out["sums"] = sflat[2:6]
        kernels.sgl_step(_dev(y), _dev(gv), _dev(xk), ptr, w, T_STEP, MU_STEP, tau, thres, theta, theta_next, out=out)
        runs.append({nm: flat[nm].cpu().numpy() for nm in names})
        runs[-1]["sums"] = sflat.cpu().numpy()
    for nm in names + ("sums",):   # two runs give identical bits
        assert np.array_equal(_bits(runs[0][nm]), _bits(runs[1][nm])), nm
    zrow = ~on1 | ~_rows(on2, ptr)
    for nm, want, bar in (("xc", xc, dxc), ("v_next", vn, dv), ("y_next", yn, dy)):
        got = runs[0][nm]
        assert np.all(got[:64] == canary) and np.all(got[64 + rows * l:] == canary), nm
        body = got[64: 64 + rows * l].reshape(rows, l)
        assert np.all(body[n:] == 0) and not np.any(np.signbit(body[n:])), nm   # rows past group_ptr[G]
        err = np.abs(body[:n].astype(LD) - want)
        assert np.all(err <= bar), (nm, float(np.max(err - bar)))
        if nm == "xc":   # zero rows and groups are exactly +0
            assert zrow.any() and (~zrow).any()
            assert np.all(body[:n][zrow] == 0) and not np.any(np.signbit(body[:n][zrow]))
            assert np.all(sr.row_norms(body[:n][~zrow].astype(np.float64)) > 0)
    s = runs[0]["sums"]
    assert np.all(s[:2] == canary) and np.all(s[6:] == canary)
    for j in range(4):
        assert abs(LD(s[2 + j]) - sums[j]) <= bars[j], (j, float(s[2 + j]), float(sums[j]), float(bars[j]))


# ------------------------------------------------------------------------------------------ 2
CERT_CASES = [(130, 3, gr.POOL_RAGGED), (475, 32, gr.POOL_SMALL), (203, 3, gr.POOL_LONG), (70, 1, (1, 2)),
              (90, 128, (1, 3, 5)), (0, 1, (1, 2))]
CERT_CASES += [(n, l, pool) for n, _, l, pool in STEP_CASES[6:]]      # (every lane layout by itself: STEP_CASES)


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CERT_CASES, ids=lambda c: "%dx%d-%s" % (c[0], c[1], c[2][-1]))
def test_sgl_certificate_step(case, dt, tau):
    from glx import kernels
    n, l, pool = case
    u = _u(dt)
    g = np.random.default_rng(23 + n + l)
    ptr = _many_groups(g, 4101, pool) if n == 0 else gr.draw_groups(g, n, pool)
    n, G = int(ptr[-1]), ptr.size - 1
    w = (np.sqrt(np.diff(ptr)) * g.uniform(0.5, 2.0, G)).astype(dt).astype(np.float64)
    mu = 0.6
    # nonzero rows, zero rows inside nonzero groups, zero groups; g on both sides of a in zero rows
    x = g.standard_normal((n, l)) * (g.random(n) < 0.5)[:, None] * _rows(g.random(G) < 0.6, ptr)[:, None]
    S = 2
    slabs = (g.standard_normal((S, n, l)) * (0.5 * mu * g.uniform(0.2, 3.0, n))[None, :, None] / np.sqrt(l)).astype(dt)
    x = x.astype(dt)
    res = kernels.sgl_certificate_step(_dev(x), _dev(slabs), ptr, w, mu, tau, want_g=True)
    gk = res["g"].cpu().numpy()
    assert np.array_equal(gk, slabs[0] + slabs[1])   # slab order, one addition
    # the reference with the kernel's own roundings of a and (1 - tau) mu
    aT, cbT = LD(dt(tau * mu)), LD(dt((1.0 - tau) * mu))
    xl, gl = x.astype(LD), gk.astype(LD)
    rho, xn = sr.row_norms(gl), sr.row_norms(xl)
    xg = gr.group_norms(xl, ptr)
    cg = cbT * w.astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        kv = gl + (aT / np.where(xn != 0, xn, 1))[:, None] * xl + _rows(cg / np.where(xg != 0, xg, 1), ptr)[:, None] * xl
    d = np.maximum(rho - aT, 0)
    nzg = _rows(xg != 0, ptr)
    rterm = np.where(nzg, np.where(xn != 0, sr.row_norms(kv), d), 0)
    ph = np.sqrt(_gsum(d * d, ptr))
    gterm = np.where(xg != 0, 0, np.maximum(ph - cg, 0))
    assert (nzg & (xn == 0)).any() and (xg == 0).any() and (xn != 0).any() and (gterm > 0).any()
    R = np.diff(ptr).astype(np.float64)
    k = R * l
    e = (k / 2 + 8) * u
    rbar = np.where(nzg, _rows(e, ptr) * (rho + aT + _rows(cg, ptr)), 0) * 1.01
    gbar = np.where(xg != 0, 0, e * (np.sqrt(_gsum(rho * rho, ptr)) + np.sqrt(R) * aT + cg)) * 1.01
    pen = LD(dt(tau)) * np.sum(xn) + LD(dt(1.0 - tau)) * np.sum(w.astype(LD) * xg)
    got = res["sums"].cpu().numpy()
    u64n = 2 * n * gr.EPS64
    assert abs(LD(got[0]) - pen) <= (float(np.max(k)) / 2 + 5) * u * pen * 1.01 + u64n * pen
    assert abs(LD(got[1]) - np.max(rho)) <= (l / 2 + 1) * u * np.max(rho) * 1.01
    terms, tbars = np.concatenate((rterm, gterm)), np.concatenate((rbar, gbar))
    assert abs(LD(got[2]) - np.max(terms)) <= np.max(tbars)
    sq = np.sum(terms * terms)
    assert abs(LD(got[3]) - sq) <= np.sum(2 * terms * tbars + tbars * tbars) + u64n * sq
    assert got[4] == float(np.sum(xg != 0)) and got[5] == float(np.sum(xn != 0))
    rn = res["row_norms"].cpu().numpy()
    assert np.all(np.abs(rn.astype(LD) - rho) <= (l / 2 + 1) * u * rho * 1.01)
    again = kernels.sgl_certificate_step(_dev(x), _dev(slabs), ptr, w, mu, tau, want_g=True)
    assert np.array_equal(_bits(again["sums"].cpu().numpy()), _bits(got))
    assert np.array_equal(_bits(again["row_norms"].cpu().numpy()), _bits(rn))


@pytest.mark.parametrize("tau", [0.0] + TAUS)
@pytest.mark.parametrize("pool", [gr.POOL_SMALL, gr.POOL_LONG, gr.POOL_RAGGED, None], ids=["small", "long", "ragged", "trips"])
def test_sgl_dual_scale(pool, tau):
    from glx import kernels
    g = np.random.default_rng(31)
    ptr = _many_groups(g, 4101, (1, 2, 3)) if pool is None else gr.draw_groups(g, 453, pool)
    n, G = int(ptr[-1]), ptr.size - 1
    w = np.sqrt(np.diff(ptr).astype(np.float64)) * g.uniform(0.5, 2.0, G)
    rho = np.abs(g.standard_normal(n)) * (g.random(n) < 0.8)
    zero = int(g.integers(G))
    rho[ptr[zero]:ptr[zero + 1]] = 0.0
    mu = 0.8
    a, cb = tau * mu, (1.0 - tau) * mu
    pads = ((1.0, 0.0), (1.0 + 3e-7, 2e-3))
    sg, smin = kernels.sgl_dual_scale(_dev(rho), ptr, w, a, cb, pads)
    sg, smin = sg.cpu().numpy(), smin.cpu().numpy()
    R = np.diff(ptr).astype(np.float64)
    for q, (mul, add) in enumerate(pads):
        p = mul * rho + add
        want = sr.exact_sg(p, ptr, w, a, cb)
        low = sr.halving_bound(p, ptr, w, a, cb)
        fin = np.isfinite(want)
        if q == 0:
            assert not fin[zero] and np.isposinf(sg[0, zero])   # a group with all-zero g
        else:
            assert fin.all()
        slack = (R[fin] + 16) * gr.EPS64 * want[fin]
        assert np.all(sg[q][fin].astype(LD) <= want[fin] + slack)
        assert np.all(sg[q][fin].astype(LD) >= want[fin] - low[fin] - slack)
        assert np.all(np.isposinf(sg[q][~fin]))
        assert smin[q] == np.min(sg[q])
        if tau == 1.0:   # a / max rho, one division
            ref = a / _gmax(p, ptr)[fin]
            assert np.all(np.abs(sg[q][fin] - ref) <= 2 * gr.EPS64 * ref)
        # the returned value is one the float64 evaluation accepts
        for kk in np.flatnonzero(fin)[:200]:
            pr = p[ptr[kk]:ptr[kk + 1]]
            v = np.maximum(sg[q][kk] * pr - a, 0)
            if cb > 0:
                assert np.sqrt(np.sum(v * v)) <= cb * w[kk] * (1 + (R[kk] + 4) * gr.EPS64)
    sg2, smin2 = kernels.sgl_dual_scale(_dev(rho), ptr, w, a, cb, pads)
    assert np.array_equal(_bits(sg2.cpu().numpy()), _bits(sg)) and np.array_equal(_bits(smin2.cpu().numpy()), _bits(smin))


# ------------------------------------------------------------------------------------------ 3
def _screen_data(pool, seed, G=None):
    g = np.random.default_rng(seed)
    ptr = _many_groups(g, G, pool) if G else gr.draw_groups(g, 453, pool)
    n, G = int(ptr[-1]), ptr.size - 1
    w = np.sqrt(np.diff(ptr).astype(np.float64)) * g.uniform(0.7, 1.4, G)
    rho = np.abs(g.standard_normal(n))
    cn = g.uniform(0.5, 2.0, n)
    gcn = np.sqrt(_gsum(cn * cn, ptr)) / w
    return ptr, w, rho, cn, gcn


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("pool", [gr.POOL_SMALL, gr.POOL_LONG, gr.POOL_RAGGED, None], ids=["small", "long", "ragged", "trips"])
def test_sgl_screen_and_expand(pool, tau):
    from glx import kernels
    torch = _torch()
    ptr, w, rho, cn, gcn = _screen_data((1, 2, 3) if pool is None else pool, 41, 4101 if pool is None else None)
    n, G = int(ptr[-1]), ptr.size - 1
    mu, s, mul, add, rad = 1.0, 0.9, 1.0 + 1e-6, 1e-3, 0.05
    a_lo, cb_lo = tau * mu * (1 - 1e-15), (1 - tau) * mu * (1 - 1e-15)
    # every test is away from equality, so float64 and longdouble agree
    p = LD(mul) * rho.astype(LD) + LD(add)
    assert np.min(np.abs(LD(s) * p + cn.astype(LD) * LD(rad) - LD(a_lo))) > 1e-9
    v = np.maximum(LD(s) * p - LD(a_lo), 0)
    assert np.min(np.abs(np.sqrt(_gsum(v * v, ptr)) / w + gcn.astype(LD) * LD(rad) - LD(cb_lo))) > 1e-9
    keep, gkeep = sr.keep_rows(rho, cn, gcn, ptr, w, s, mul, add, rad, a_lo, cb_lo, tau < 1.0)
    per = _gsum(keep.astype(np.int64), ptr)
    sizes = np.diff(ptr)
    assert ((per > 0) & (per < sizes)).any()        # a group that loses interior rows
    assert ((per == 0) & (sizes > 1)).any()         # a group that loses all its rows
    res = kernels.sgl_screen(_dev(rho), _dev(cn), _dev(gcn), ptr, w, s, mul, add, rad, a_lo, cb_lo, tau < 1.0)
    assert np.array_equal(res["keep"].cpu().numpy(), keep.astype(np.int32))
    assert np.array_equal(res["group_keep"].cpu().numpy(), gkeep.astype(np.int32))
    assert res["counts"].cpu().tolist() == [float(gkeep.sum()), float(keep.sum())]
    gmap = np.arange(G, dtype=np.int32)[::-1].copy() + 7
    for km, mp in ((res["keep"], None), (res["keep"], gmap), (torch.zeros(n, dtype=torch.int32, device="cuda"), None),
                   (torch.ones(n, dtype=torch.int32, device="cuda"), gmap)):
        out = kernels.sgl_expand(km, _dev(ptr), _dev(w), _dev(gcn), None if mp is None else _dev(mp))
        rows, nptr, nw, ngcn, nmap, cnt = sr.expand_lists(km.cpu().numpy(), ptr, w, gcn, mp)
        K = cnt[0]
        assert out["count"].cpu().tolist() == cnt
        got_rows = out["rows"].cpu().numpy()
        assert np.array_equal(got_rows[:cnt[3]], rows) and np.all(got_rows[cnt[3]:] == -2)
        assert np.array_equal(out["group_ptr"].cpu().numpy()[:K + 1], nptr)
        assert np.all(out["group_ptr"].cpu().numpy()[K + 1:] == -2)
        assert np.array_equal(out["weights"].cpu().numpy()[:K], nw) and np.array_equal(out["gcn"].cpu().numpy()[:K], ngcn)
        assert np.array_equal(out["map"].cpu().numpy()[:K], nmap) and np.all(out["map"].cpu().numpy()[K:] == -2)
    # nothing is kept: s = 0 and no radius put every row below a_lo (tau > 0)
    none = kernels.sgl_screen(_dev(rho), _dev(cn), _dev(gcn), ptr, w, 0.0, mul, add, 0.0, a_lo, cb_lo, tau < 1.0)
    assert int(none["keep"].sum()) == 0 and none["counts"].cpu().tolist() == [0.0, 0.0]
    # NaN keeps everything
    nan = kernels.sgl_screen(_dev(rho), _dev(cn), _dev(gcn), ptr, w, float("nan"), mul, add, rad, a_lo, cb_lo, tau < 1.0)
    assert int(nan["keep"].sum()) == n and nan["counts"].cpu().tolist() == [float(G), float(n)]


# ------------------------------------------------------------------------------------------ 4
def _round_slack(ref, dt):
    """How far a primal or dual value composed in dt arithmetic may be from the exact one: the reference's own
    gap plus (m + n) l roundings of the objective's size."""
    m, n = ref["A"].shape
    l = ref["b"].shape[1]
    return float(ref["gap"]) + 8 * (m + n) * l * _u(dt) * abs(float(ref["primal"]))


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: "%dx%dx%d-%s-%g" % (c[0], c[1], c[2], c[3][-1], c[4]))
def test_certificate_brackets_the_optimum(case):
    import glx
    ref = sr.reference_solution(*case)
    g = np.random.default_rng(3)
    slack = _round_slack(ref, np.float64)
    for x in (ref["x"], ref["x"] * (1 + 0.05 * g.standard_normal(ref["x"].shape)), None):
        c = glx.certificate(x, ref["A"], ref["b"], ref["mu"], groups=ref["ptr"], weights=ref["w"], row_ratio=ref["tau"],
                            row_norms=True)
        assert c["dual"] <= float(ref["primal"]) + slack and float(ref["dual"]) - slack <= c["primal"]
        xx = np.zeros_like(ref["x"]) if x is None else x
        want = sr.certificate(xx.astype(LD), ref["A"].astype(LD), ref["b"].astype(LD), LD(ref["mu"]), ref["ptr"],
                              ref["w"], ref["tau"])
        tol = 1e-9 * abs(float(want["primal"]))
        assert abs(c["primal"] - float(want["primal"])) <= tol and abs(c["dual"] - float(want["dual"])) <= tol
        assert abs(c["scale_min"] - float(want["s_min"])) <= 1e-9 * float(want["s_min"])
        assert c["nonzero_rows"] == want["nonzero_rows"] and c["nonzero_groups"] == want["nonzero_groups"]
        assert abs(c["kkt_max"] - float(want["kkt_max"])) <= 1e-9 * (float(want["kkt_max"]) + ref["mu"])
        assert np.allclose(c["row_norms"], np.asarray(want["row_norms"], dtype=np.float64), rtol=1e-9, atol=1e-12)
        assert c["row_ratio"] == ref["tau"] and c["fused"] is False and "k_sgl_cert" in c["plan"]
    at = glx.certificate(ref["x"], ref["A"], ref["b"], ref["mu"], groups=ref["ptr"], weights=ref["w"],
                         row_ratio=ref["tau"])
    assert at["rel_gap"] <= 1e-9


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_certificate_tau1_is_the_row_certificate_and_tau0_todays(dt):
    import glx
    ref = sr.reference_solution(*sr.CASES[0], f32=dt == np.float32)
    A, b = ref["A"].astype(dt), ref["b"].astype(dt)
    x = (ref["x"] * 1.01).astype(dt)
    u = _u(dt)
    l = b.shape[1]
    one = glx.certificate(x, A, b, ref["mu"], groups=ref["ptr"], weights=ref["w"], row_ratio=1.0)
    row = glx.certificate(x, A, b, ref["mu"])
    # the same residual and g; the row norms differ by the order of an l-term sum, both sides: (l / 2 + 2) u each
    e = 4 * (l / 2 + 8) * u
    assert one["primal"] == pytest.approx(row["primal"], rel=e) and one["nonzero_rows"] == row["nonzero_rows"]
    assert one["scale"] == pytest.approx(row["scale"], rel=e)
    assert abs(one["dual"] - row["dual"]) <= e * (abs(row["dual"]) + abs(row["primal"]))
    assert abs(one["kkt_max"] - row["kkt_max"]) <= e * (row["gmax"] + 2 * ref["mu"])
    assert abs(one["kkt_fro"] - row["kkt_fro"]) <= e * np.sqrt(A.shape[1]) * (row["gmax"] + 2 * ref["mu"])
    for rr in (0, 0.0):
        zero = glx.certificate(x, A, b, ref["mu"], groups=ref["ptr"], weights=ref["w"], row_ratio=rr, row_norms=True)
        today = glx.certificate(x, A, b, ref["mu"], groups=ref["ptr"], weights=ref["w"], row_norms=True)
        assert set(zero) == set(today)
        for key in today:
            if key == "group_norms":
                assert np.array_equal(_bits(zero[key]), _bits(today[key]))
            else:
                assert zero[key] == today[key], key
    assert glx.mu_max(A, b, groups=ref["ptr"], weights=ref["w"], row_ratio=0) == \
        glx.mu_max(A, b, groups=ref["ptr"], weights=ref["w"])


# ------------------------------------------------------------------------------------------ 5
def _dist(ref, x):
    return float(np.linalg.norm(ref["A"].astype(LD) @ (np.asarray(x, dtype=LD) - ref["x"].astype(LD))))


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: "%dx%dx%d-%s-%g" % (c[0], c[1], c[2], c[3][-1], c[4]))
def test_solve_certified(case):
    import glx
    ref = sr.reference_solution(*case)
    tol = 1e-8
    kw = dict(groups=ref["ptr"], weights=ref["w"], row_ratio=ref["tau"], tol=tol)
    x, info = glx.solve_certified(ref["A"], ref["b"], ref["mu"], **kw)
    xu, iu = glx.solve_certified(ref["A"], ref["b"], ref["mu"], screen=False, **kw)
    slack = _round_slack(ref, np.float64)
    for xx, ii in ((x, info), (xu, iu)):
        assert ii["converged"] and ii["rel_gap"] <= tol and ii["row_ratio"] == ref["tau"]
        assert ii["primal"] >= float(ref["dual"]) - slack and ii["dual"] <= float(ref["primal"]) + slack
        assert _dist(ref, xx) <= np.sqrt(2 * max(ii["gap"], 0) + 2 * slack) + np.sqrt(2 * slack)
        assert "k_sgl_fista" in ii["plan"]
    assert float(np.linalg.norm(ref["A"] @ (x - xu))) <= np.sqrt(2 * info["gap"] + 2 * slack) + np.sqrt(2 * iu["gap"] + 2 * slack)
    # no row of the reference support is ever absent from kept_rows
    kept = np.zeros(ref["x"].shape[0], dtype=bool)
    kept[info["kept_rows"]] = True
    assert np.all(kept[ref["support"]])
    gk = np.zeros(ref["ptr"].size - 1, dtype=bool)
    gk[info["kept_groups"]] = True
    assert np.all(gk[gr.group_norms(ref["x"], ref["ptr"]) != 0])
    assert np.all(x[~kept] == 0) and not np.any(np.signbit(x[~kept]))
    assert info["compactions"] >= 1 and len(info["kept_row_history"]) == info["compactions"]
    h = info["kept_row_history"]
    assert all(b_ <= a_ for a_, b_ in zip(h, h[1:])) and h[-1] >= int(ref["support"].sum())
    hg = info["kept_history"]
    assert all(b_ <= a_ for a_, b_ in zip(hg, hg[1:])) and all(r_ >= g_ for r_, g_ in zip(h, hg))
    assert info["kept_rows"].size < ref["x"].shape[0]
    assert info["nonzero_rows"] == int(np.sum(sr.row_norms(x) != 0))
    # an unscreened iteration makes exactly two passes over A (every check and final certificate two more)
    assert iu["passes"] == 2.0 * (iu["iterations"] + iu["checks"] + iu["rounds"])
    assert iu["kept_rows"].size == ref["x"].shape[0] and iu["kept_row_history"] == []


def test_solve_certified_f32():
    import glx
    ref = sr.reference_solution(*sr.CASES[0], f32=True)
    A, b = ref["A"].astype(np.float32), ref["b"].astype(np.float32)
    tol = 1e-4
    x, info = glx.solve_certified(A, b, ref["mu"], groups=ref["ptr"], weights=ref["w"], row_ratio=ref["tau"], tol=tol)
    assert x.dtype == np.float32 and info["converged"] and info["rel_gap"] <= tol
    slack = _round_slack(ref, np.float32)
    assert _dist(ref, x) <= np.sqrt(2 * max(info["gap"], 0) + 2 * slack) + np.sqrt(2 * slack)
    kept = np.zeros(ref["x"].shape[0], dtype=bool)
    kept[info["kept_rows"]] = True
    # (how much float32 screens is not asserted: the guard's gamma_n ||A||_F ||x|| term of the radius can
    # outweigh the row threshold tau mu; only safety is)
    assert np.all(kept[ref["support"]]) and np.all(x[~kept] == 0)


@pytest.mark.parametrize("tau", TAUS)
def test_path(tau):
    import glx
    m, n, l, pool = 40, 130, 3, gr.POOL_RAGGED
    A, b, ptr, w = sr.instance(sr.SEED, m, n, l, pool)
    top = glx.mu_max(A, b, groups=ptr, weights=w, row_ratio=tau)
    assert top == pytest.approx(sr.mu_max(A, b, ptr, w, tau), rel=1e-10)
    entries = glx.path(A, b, n_mus=4, mu_min_ratio=0.1, groups=ptr, weights=w, row_ratio=tau, tol=1e-7)
    mu0, x0, i0 = entries[0]
    assert mu0 == top and not np.any(x0) and i0["iterations"] == 0 and i0["converged"]
    nz = []
    for mu, x, info in entries:
        assert info["converged"] and info["rel_gap"] <= 1e-7
        want = sr.certificate(x.astype(LD), A.astype(LD), b.astype(LD), LD(mu), ptr, w, tau)
        assert float(want["rel_gap"]) <= 1e-7 * (1 + 1e-6) + 1e-12
        h = info["kept_row_history"]
        assert all(b_ <= a_ for a_, b_ in zip(h, h[1:]))
        nz.append(info["nonzero_rows"])
    assert nz[0] == 0 and nz[-1] > 0
    below = glx.certificate(None, A, b, 0.999 * top, groups=ptr, weights=w, row_ratio=tau)
    assert below["scale"] < 1.0 and below["kkt_max"] > 0.0


# ------------------------------------------------------------------------------------------ 6
def test_zero_one_sample_weights_are_the_row_subset():
    import glx
    ref = sr.reference_solution(*sr.CASES[2])
    A, b = ref["A"], ref["b"]
    g = np.random.default_rng(9)
    sw = (g.random(A.shape[0]) < 0.7).astype(np.float64)
    on = sw > 0
    tau = ref["tau"]
    kw = dict(groups=ref["ptr"], weights=ref["w"], row_ratio=tau, tol=1e-9)
    top_w = glx.mu_max(A, b, groups=ref["ptr"], weights=ref["w"], sample_weight=sw, row_ratio=tau)
    top_s = glx.mu_max(A[on], b[on], groups=ref["ptr"], weights=ref["w"], row_ratio=tau)
    assert top_w == pytest.approx(top_s, rel=1e-10)
    mu = 0.3 * top_s
    xw, iw = glx.solve_certified(A, b, mu, sample_weight=sw, **kw)
    xs, is_ = glx.solve_certified(A[on], b[on], mu, **kw)
    assert iw["converged"] and is_["converged"]
    assert iw["primal"] == pytest.approx(is_["primal"], rel=1e-7)
    assert float(np.linalg.norm(A[on] @ (xw - xs))) <= np.sqrt(2 * iw["gap"]) + np.sqrt(2 * is_["gap"]) + 1e-9
    cw = glx.certificate(xs, A, b, mu, groups=ref["ptr"], weights=ref["w"], row_ratio=tau, sample_weight=sw)
    cs = glx.certificate(xs, A[on], b[on], mu, groups=ref["ptr"], weights=ref["w"], row_ratio=tau)
    for key in ("primal", "dual", "kkt_max", "scale_min"):
        assert cw[key] == pytest.approx(cs[key], rel=1e-10, abs=1e-12), key


def test_cv_path():
    import glx
    A, b, ptr, w = sr.instance(sr.SEED, 60, 130, 3, gr.POOL_RAGGED)
    cv = glx.cv_path(A, b, folds=3, n_mus=4, mu_min_ratio=0.05, groups=ptr, weights=w, row_ratio=0.3, tol=1e-6)
    assert cv["mus"][0] == glx.mu_max(A, b, groups=ptr, weights=w, row_ratio=0.3)
    assert cv["mu_best"] in cv["mus"] and cv["mu_one_se"] in cv["mus"] and cv["fold_loss"].shape == (3, 4)
    assert np.all(np.isfinite(cv["fold_loss"])) and np.all(cv["fold_loss"] > 0)
    assert all(i["converged"] and i["row_ratio"] == 0.3 for f in cv["info"] for i in f)
    assert cv["best"] > 0   # some fit beats x = 0 on held-out rows


# ------------------------------------------------------------------------------------------ 7
def test_refusals():
    import glx
    from glx import _lib, kernels
    A, b, ptr, w = sr.instance(sr.SEED, 40, 130, 3, gr.POOL_RAGGED)
    for fn in (lambda: glx.solve_certified(A, b, 1.0, groups=ptr, row_ratio=0.5, fit_intercept=True),
               lambda: glx.certificate(None, A, b, 1.0, groups=ptr, row_ratio=0.5, fit_intercept=True),
               lambda: glx.path(A, b, groups=ptr, row_ratio=0.5, fit_intercept=True)):
        with pytest.raises(ValueError, match="fit_intercept"):
            fn()
    x = _dev(np.zeros((130, 3)))
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(_lib.GlxError, match="row_ratio"):
            kernels.sgl_step(x, x, x, ptr, w, 0.3, 0.7, bad, 1e-300, 0.5, 0.4)
        with pytest.raises(_lib.GlxError, match="row_ratio"):
            kernels.sgl_certificate_step(x, x, ptr, w, 0.7, bad)
    rec = (ctypes.c_double * 12)()
    with pytest.raises(_lib.GlxError, match="row_ratio"):
        _lib.check(_lib.lib().glx_sgl_certificate(_lib.GLX_F64, 40, 130, 3, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1.0,
                                                  2.0, ptr.size - 1, ptr.ctypes.data, w.ctypes.data, None, None, rec,
                                                  x.data_ptr(), 1 << 30, None))
