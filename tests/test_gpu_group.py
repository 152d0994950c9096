"""Feature groups and weights on the GPU: the four kernels one launch at a time, whole certified
solves on groups, two oracles that need no new reference, the path and the refusals. Reference:
tests/group_ref.py. u = eps / 2 is the unit roundoff of the working dtype T, u64 that of float64;
k = size_g l is the number of elements of a group; every bar below is first order in u times
(1 + 4 e) with e the largest relative error it composes, which covers the products of errors.

1. group_step (k_group_fista) against group_ref.step_ref, longdouble on the same T inputs. Each
   group's ||w_[g]|| is placed at t mu w_g (1 +- d), d in [0.05, 0.5], by scaling its y and g, so no
   group flips side and the cancellation in c = ||w|| - t mu w_g is bounded by 1 / d. Roundings:
     w_e = y_e - t g_e            a product and a subtraction: |dw_e| <= a_e = u (2 |t g_e| + |w_e|)
     nrm = sqrt(sum w_e^2)        a k-term sum of squares, halved by the root, and the root:
                                  e_n = (k / 2 + 1) u + ||a||_2 / nrm relative
     t mu w_g                     one product: u relative
     c = nrm - t mu w_g           one subtraction; relative to c = t mu w_g d:
                                  e_c = ((1 + d) e_n + u) / d + u          (the 1 / d amplification)
     xc_e = (w_e c) / nrm         one product, one division:
                                  |dxc_e| <= (c / nrm) a_e + |xc_e| (e_c + e_n + 2 u)
   and xc = 0 exactly on the other side of the threshold. Then per element
     v_e = xo + (xc - xo) / theta:    dv = (dxc + u |xc - xo|) / theta + u |xc - xo| / theta + u |v|
     y+_e = a1 xc + b1 v:             dy = |a1| (dxc + u |xc|) + |b1| (dv + u |v|) + u |y+|
   and the sums, accumulated in double (their own rounding, n l u64 relative, is added):
     sum g (xc - y):   sum |g| (dxc + u |xc - y|) + u |g (xc - y)|
     sum (xc - y)^2:   sum 2 |xc - y| (dxc + u |xc - y|) + u (xc - y)^2
     sum w_g ||xc_g||: sum w_g (||dxc_g||_2 + ((k / 2 + 1) u + u) ||xc_g||)
     max |xc|:         max dxc
2. group_certificate_step, group_cnorm, group_expand. A k-term norm is (k / 2 + 1) u relative, the
   division by w_g one more u; kkt of a nonzero group: k_e = g_e + (mu w_g x_e) / ||x|| has a product
   for mu w_g, a product, a division by a norm ((k / 2 + 1) u) and a sum, so
   |dk_e| <= |mu w_g x_e / ||x||| (k / 2 + 4) u + u |k_e| and kkt is off by ||dk||_2 + (k / 2 + 1) u kkt;
   of a zero group, max(||g|| - mu w_g, 0): (k / 2 + 1) u ||g|| + u mu w_g + u kkt. gcn is within the
   k_col_norms bar, (m + 2) u64 relative, plus max_run + 3 roundings. The lists of group_expand are
   exactly NumPy's.
3. Whole solves against group_ref.reference_solution. Slack of the objective comparisons: the
   reference's own gap plus group_ref.primal_bar (the group guard's item 2).
4. Oracles: size-1 groups of weight 1 against the row path (the record's entries differ only by the
   order of an l-term norm's sum and the weight's product, both sides: twice (l / 2 + 2) u on the
   norms; kkt per row twice (l / 2 + 5) u (||g_i|| + 2 mu), item 2's worst case); weights on single
   rows against the row solve of A / w.
5. The path on groups. 6. Refusals through the C ABI.

Layouts and trips. A team of LPG lanes owns a group; group_dispatch picks LPG and the elements per
lane from the longest run's max_run l elements: <= 4: 4 lanes, <= 16: 16, <= 32: 32, <= 64: a wave,
one element per lane; <= 128, 256, 512: a wave with 2, 4, 8 per lane; longer: two sweeps. The grid
is capped at 1024 workgroups, 1024 * 256 / LPG groups a trip. STEP_CASES and CERT_CASES hold one
case per layout in one trip of at most 34 workgroups. SEVERAL_TRIPS holds one case per layout
family with G five past one trip (two trips, the second ragged): (l, pool, G) = (2, (1, 2), 65541)
at 4 lanes, (16, (3, 4), 4101) at a wave with one element per lane and (64, (2, 8, 9), 4101) at two
sweeps, for group_step (rows = n + 63, the widest padding the entry takes, so the loop over the rows
past group_ptr[G] stays within one trip there; the (200, 256, 128) case of STEP_CASES makes two
trips of it on its 19 workgroups) and for group_certificate_step; group_cnorm runs G = 262149 with
a lane per group (runs <= 8) and G = 4101 with a wave per group (runs of 9 .. 12). In each, the
groups on both sides of the trip boundary, which hold one of the longest run, run again as a
problem of their own and give the same bits. group_expand is one workgroup; its case with 573
kept groups of 257 .. 260 rows fills the 512-entry list of long groups and reaches the fallback.
"""
import ctypes
import functools

import numpy as np
import pytest

import group_ref as gr

pytestmark = pytest.mark.gpu

LD = gr.LD
TOL = 1e-8


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


def _rows(v, ptr):
    return gr.expand_rows(v, ptr)


# ------------------------------------------------------------------------------------------ 1
STEP_CASES = [(475, 512, 16, gr.POOL_SMALL), (475, 512, 16, gr.POOL_LONG), (130, 192, 3, gr.POOL_RAGGED),
              (130, 130, 3, gr.POOL_RAGGED), (70, 70, 1, (1, 2)), (200, 256, 128, (1, 3, 5)),
              (100, 128, 16, (1, 2)), (100, 100, 16, (3, 4)), (100, 128, 32, (5, 8)), (100, 128, 64, (2, 8))]
# (runs of at most 15, 2, 32, 64, 128, 256, 512 elements: one case per in-register layout; 640 and 1040: two sweeps)
T_STEP, MU_STEP = 0.3, 0.7


def _draw_groups_at_once(g, G, pool):
    """G sizes from `pool` in one call (the several-trip cases): group_ptr, int32; n = group_ptr[G]."""
    return np.concatenate(([0], np.cumsum(g.choice(pool, size=G)))).astype(np.int32)


def _lpg(max_len):
    """Lanes per group of group_dispatch for a longest run of max_len elements (EPL: 1 up to 64
    elements, then 2, 4, 8 in registers up to 512, then the two-sweep form)."""
    return 4 if max_len <= 4 else 16 if max_len <= 16 else 32 if max_len <= 32 else 64


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _step_inputs(n, rows, l, pool, dt, seed, ptr=None):
    """y, g, xk (rows x l, T) with every group's ||y - t g|| at t mu w_g (1 +- d); one group all zero."""
    g = np.random.default_rng(seed)
    if ptr is None:
        ptr = gr.draw_groups(g, n, pool)
    G = ptr.size - 1
    w = np.sqrt(np.diff(ptr).astype(np.float64)) * g.uniform(0.5, 2.0, G)
    y = g.standard_normal((rows, l))
    gv = g.standard_normal((rows, l))
    xk = g.standard_normal((rows, l)) * (g.random((rows, l)) < 0.7)
    d = g.uniform(0.06, 0.49, G) * np.where(g.random(G) < 0.5, 1.0, -1.0)
    wv = (y - T_STEP * gv)[:n]
    nrm = np.asarray(gr.group_norms(wv, ptr))
    alpha = _rows(T_STEP * MU_STEP * w * (1.0 + d) / nrm, ptr)[:, None]
    y[:n] *= alpha
    gv[:n] *= alpha
    zero = int(g.integers(G))
    y[ptr[zero]:ptr[zero + 1]] = 0.0
    gv[ptr[zero]:ptr[zero + 1]] = 0.0
    return ptr, w, y.astype(dt), gv.astype(dt), xk.astype(dt), zero


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "%d(%d)x%d-%s" % (c[0], c[1], c[2], c[3][-1]))
def test_group_step(case, dt):
    _step_case(case, dt)


def _step_case(case, dt, ptr=None):
    """One group_step launch with all the checks of test 1; ptr: a description drawn beforehand.
    Returns the description, the inputs and the outputs."""
    from glx import kernels
    torch = _torch()
    n, rows, l, pool = case
    u = _u(dt)
    ptr, w, y, gv, xk, zero = _step_inputs(n, rows, l, pool, dt, 7 + n + l, ptr)
    thres = float(np.finfo(dt).tiny)
    theta, theta_next = 2.0 / 4, 2.0 / 5
    xc, vn, yn, sums, nrm, tmuw = gr.step_ref(y[:n], gv[:n], xk[:n], ptr, w, T_STEP, MU_STEP, thres, theta, theta_next)
    dd = np.abs(nrm / np.where(tmuw > 0, tmuw, 1) - 1)
    live = np.ones(ptr.size - 1, dtype=bool)
    live[zero] = False
    assert np.all(dd[live] >= 0.05) and np.all(dd[live] <= 0.5)   # the construction holds after rounding to T
    # the bars of the module docstring
    k = np.diff(ptr).astype(np.float64) * l
    tl = LD(dt(T_STEP))
    yl, gl, xl = y[:n].astype(LD), gv[:n].astype(LD), xk[:n].astype(LD)
    wv = yl - tl * gl
    a = u * (2 * np.abs(tl * gl) + np.abs(wv))
    an = np.sqrt(_gsum(np.sum(a * a, axis=1), ptr))
    safe = np.where(nrm > 0, nrm, 1)
    e_n = (k / 2 + 1) * u + an / safe
    on = nrm > tmuw
    e_c = np.where(on, ((1 + dd) * e_n + u) / np.where(dd > 0, dd, 1) + u, 0)
    lift = 1 + 4 * float(np.max(e_c + e_n))
    cd = np.where(on, (nrm - tmuw) / safe, 0)
    dxc = (_rows(cd, ptr)[:, None] * a + np.abs(xc) * _rows(e_c + e_n + 2 * u, ptr)[:, None]) * lift
    th, a1, b1 = LD(dt(theta)), LD(dt(1.0 - theta_next)), LD(dt(theta_next))
    xo = np.where(np.abs(xl) < LD(thres), 0, xl)
    dv = ((dxc + u * np.abs(xc - xo)) / th + u * np.abs(xc - xo) / th + u * np.abs(vn)) * lift
    dy = (abs(a1) * (dxc + u * np.abs(xc)) + abs(b1) * (dv + u * np.abs(vn)) + u * np.abs(yn)) * lift
    dl = xc - yl
    u64n = n * l * gr.EPS64 / 2
    wT = w.astype(dt).astype(LD)
    xcn = gr.group_norms(xc, ptr)
    bars = [np.sum(np.abs(gl) * (dxc + u * np.abs(dl)) + u * np.abs(gl * dl)) * lift + u64n * np.sum(np.abs(gl * dl)),
            np.sum(2 * np.abs(dl) * (dxc + u * np.abs(dl)) + u * dl * dl) * lift + u64n * np.sum(dl * dl),
            np.sum(wT * (np.sqrt(_gsum(np.sum(dxc * dxc, axis=1), ptr)) + ((k / 2 + 1) * u + u) * xcn)) * lift
            + u64n * np.sum(wT * xcn),
            np.max(dxc)]
    # canaries around every output
    canary = -7.5
    names = ("xc", "v_next", "y_next")
    flat = {nm: torch.full((64 + rows * l + 64,), canary, dtype=torch.float64 if dt == np.float64 else torch.float32,
                           device="cuda") for nm in names}
    out = {nm: flat[nm][64: 64 + rows * l].view(rows, l) for nm in names}
    sflat = torch.full((8,), canary, dtype=torch.float64, device="cuda")
    out["sums"] = sflat[2:6]
    res = kernels.group_step(_dev(y), _dev(gv), _dev(xk), ptr, w, T_STEP, MU_STEP, thres, theta, theta_next, out=out)
    for nm, want, bar in (("xc", xc, dxc), ("v_next", vn, dv), ("y_next", yn, dy)):
        got = flat[nm].cpu().numpy()
        assert np.all(got[:64] == canary) and np.all(got[64 + rows * l:] == canary), nm
        body = got[64: 64 + rows * l].reshape(rows, l)
        assert np.all(body[n:] == 0) and not np.any(np.signbit(body[n:])), nm   # rows past group_ptr[G]
        err = np.abs(body[:n].astype(LD) - want)
        assert np.all(err <= bar), (nm, float(np.max(err / np.maximum(bar, LD(1e-300)))))
        if nm == "xc":
            assert np.all(body[:n][_rows(~on, ptr)] == 0)           # the other side of the threshold: exactly 0
    sg = sflat.cpu().numpy()
    assert np.all(sg[:2] == canary) and np.all(sg[6:] == canary)
    for j in range(4):
        assert abs(LD(sg[2 + j]) - sums[j]) <= bars[j], (j, float(sg[2 + j]), float(sums[j]), float(bars[j]))
    print("\n%s %s: max err / bar xc %.3f" % (case[:3], dt.__name__, float(np.max(
        np.abs(flat["xc"].cpu().numpy()[64: 64 + rows * l].reshape(rows, l)[:n].astype(LD) - xc)
        / np.maximum(dxc, LD(1e-300))))))
    # slabs are summed in slab order: bit-equal to the step on their sum in T, and run to run
    parts = np.stack([gv * dt(0.5), gv * dt(0.25), gv * dt(0.25)])
    summed = (parts[0] + parts[1]) + parts[2]
    r1 = kernels.group_step(_dev(y), _dev(parts), _dev(xk), ptr, w, T_STEP, MU_STEP, thres, theta, theta_next)
    r2 = kernels.group_step(_dev(y), _dev(summed), _dev(xk), ptr, w, T_STEP, MU_STEP, thres, theta, theta_next)
    for nm in ("xc", "v_next", "y_next", "sums"):
        assert torch.equal(r1[nm], r2[nm]), nm
    if np.array_equal(summed, gv):
        for nm in ("xc", "v_next", "y_next", "sums"):
            assert torch.equal(r1[nm].reshape(-1), res[nm].reshape(-1)), nm
    return ptr, w, y, gv, xk, res, (thres, theta, theta_next)


# One case per layout family past one trip of the 1024-workgroup grid (1024 * 256 / LPG groups),
# (l, pool, G): 4 lanes per group (65536 groups a trip), a wave per group with one element per lane in
# registers (4096 a trip), the two-sweep form (4096 a trip; about 1.7 M elements). Two trips each, the
# second of 5 groups. rows = n + 63, the widest padding the entry takes.
SEVERAL_TRIPS = [(2, (1, 2), 65541), (16, (3, 4), 4101), (64, (2, 8, 9), 4101)]
SEVERAL_IDS = ["4-lanes", "wave-1-per-lane", "two-sweeps"]


def _trip_slice(ptr, l, pool):
    """The groups on both sides of the trip boundary: (first group, its first row); they hold a
    group of the longest run, so on their own they take the same layout."""
    G = ptr.size - 1
    per_trip = 1024 * 256 // _lpg(max(pool) * l)
    assert -(-G // per_trip) == 2 and 0 < G - per_trip < 40     # a second trip of a few groups
    g0 = per_trip - 40
    assert np.diff(ptr[g0:]).max() == max(pool) == np.diff(ptr).max()
    return g0, int(ptr[g0])


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("l,pool,G", SEVERAL_TRIPS, ids=SEVERAL_IDS)
def test_group_step_several_trips(l, pool, G, dt):
    """Test 1 past one trip. Its bars hold as they stand: the sums' accumulation term is the
    worst case of an n l-term sum, whatever the trips. Then the groups on both sides of the trip
    boundary run again as a problem of their own, in one trip: a group's outputs depend on neither
    G nor the trip, so they come back bit for bit (NaN-filled by the wrapper before the launch)."""
    from glx import kernels
    ptr = _draw_groups_at_once(np.random.default_rng(1000 * l + G), G, pool)
    n = int(ptr[-1])
    g0, r0 = _trip_slice(ptr, l, pool)
    ptr, w, y, gv, xk, res, (thres, theta, theta_next) = _step_case((n, n + 63, l, pool), dt, ptr=ptr)
    part = kernels.group_step(_dev(y[r0:n]), _dev(gv[r0:n]), _dev(xk[r0:n]), ptr[g0:] - ptr[g0], w[g0:], T_STEP,
                              MU_STEP, thres, theta, theta_next)
    for nm in ("xc", "v_next", "y_next"):
        assert np.array_equal(_bits(part[nm].cpu().numpy()), _bits(res[nm].cpu().numpy()[r0:n])), nm


# ------------------------------------------------------------------------------------------ 2
CERT_CASES = [(512, 16, gr.POOL_SMALL), (512, 16, gr.POOL_LONG), (130, 3, gr.POOL_RAGGED), (70, 1, (1, 2)),
              (200, 128, (1, 3, 5)), (100, 16, (1, 2)), (100, 16, (3, 4)), (100, 32, (5, 8)), (100, 64, (2, 8))]


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CERT_CASES, ids=lambda c: "%dx%d-%s" % (c[0], c[1], c[2][-1]))
def test_group_certificate_step(case, dt):
    _cert_case(case, dt)


def _cert_case(case, dt, ptr=None):
    """One group_certificate_step launch with all the checks of test 2; ptr: a description drawn
    beforehand. Returns the description, the inputs and the outputs."""
    from glx import kernels
    torch = _torch()
    n, l, pool = case
    u = _u(dt)
    g = np.random.default_rng(31 + n + l)
    if ptr is None:
        ptr = gr.draw_groups(g, n, pool)
    G = ptr.size - 1
    w = np.sqrt(np.diff(ptr).astype(np.float64)) * g.uniform(0.5, 2.0, G)
    mu = 0.8
    x = (g.standard_normal((n, l)) * _rows(g.random(G) < 0.4, ptr)[:, None]).astype(dt)
    gv = (g.standard_normal((n, l)) * _rows(g.uniform(0.2, 2.0, G), ptr)[:, None]).astype(dt)
    xl, gl = x.astype(LD), gv.astype(LD)
    wT = w.astype(dt).astype(LD)
    muw = LD(dt(mu)) * wT
    gn, xn = gr.group_norms(gl, ptr), gr.group_norms(xl, ptr)
    nz = xn != 0
    assert 0 < nz.sum() < G
    t2 = _rows(np.where(nz, muw / np.where(nz, xn, 1), 0), ptr)[:, None] * xl
    kv = gl + t2
    kn = gr.group_norms(kv, ptr)
    kkt = np.where(nz, kn, np.maximum(gn - muw, 0))
    k = np.diff(ptr).astype(np.float64) * l
    e_k = (k / 2 + 1) * u
    dk = np.abs(t2) * _rows(k / 2 + 4, ptr)[:, None] * u + u * np.abs(kv)
    dkkt = np.where(nz, np.sqrt(_gsum(np.sum(dk * dk, axis=1), ptr)) + e_k * kn, e_k * gn + u * muw + u * kkt)
    dkkt = dkkt * (1 + 4 * float(np.max(e_k)))
    gq = gn / wT
    dgq = (e_k + u) * gq * (1 + 4 * float(np.max(e_k)))
    u64n = G * gr.EPS64 / 2
    want = [np.sum(wT * xn), np.max(gq), np.max(kkt), np.sum(kkt * kkt), LD(nz.sum())]
    bars = [np.sum(wT * xn * (e_k + u)) * (1 + 4 * float(np.max(e_k))) + u64n * want[0], np.max(dgq), np.max(dkkt),
            np.sum(2 * kkt * dkkt + dkkt * dkkt) + u64n * want[3], 0]
    out = kernels.group_certificate_step(_dev(x), _dev(gv), ptr, w, mu, want_g=True)
    got = out["sums"].cpu().numpy()
    for j in range(5):
        assert abs(LD(got[j]) - want[j]) <= bars[j], (j, float(got[j]), float(want[j]), float(bars[j]))
    rn = out["group_norms"].cpu().numpy()
    assert np.all(np.abs(rn.astype(LD) - gq) <= dgq)
    assert got[1] == rn.max()                                     # the maximum is that of the stored figures
    assert np.array_equal(out["g"].cpu().numpy(), gv)
    parts = np.stack([gv * dt(0.5), gv * dt(0.5)])
    if np.array_equal(parts[0] + parts[1], gv):
        again = kernels.group_certificate_step(_dev(x), _dev(parts), ptr, w, mu, want_g=True)
        for key in ("sums", "group_norms", "g"):
            assert torch.equal(again[key], out[key]), key
    # NaN handling is cert_row's: a NaN in x reaches the count and the sums fed by that group
    xb = x.copy()
    first = int(np.nonzero(nz)[0][0])
    xb[ptr[first], 0] = np.nan
    bad = kernels.group_certificate_step(_dev(xb), _dev(gv), ptr, w, mu)["sums"].cpu().numpy()
    assert np.isnan(bad[0]) and np.isnan(bad[2]) and np.isnan(bad[4]) and bad[1] == got[1]
    return ptr, w, x, gv, mu, out


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("l,pool,G", SEVERAL_TRIPS, ids=SEVERAL_IDS)
def test_group_certificate_step_several_trips(l, pool, G, dt):
    """Test 2 past one trip, with its bars as they stand (the sums' accumulation term is the worst case
    of a G-term sum), then the groups on both sides of the trip boundary as a problem of their own:
    ||g_[g]|| / w_g and the summed gradient come back bit for bit."""
    from glx import kernels
    ptr = _draw_groups_at_once(np.random.default_rng(2000 * l + G), G, pool)
    n = int(ptr[-1])
    g0, r0 = _trip_slice(ptr, l, pool)
    ptr, w, x, gv, mu, out = _cert_case((n, l, pool), dt, ptr=ptr)
    part = kernels.group_certificate_step(_dev(x[r0:]), _dev(gv[r0:]), ptr[g0:] - ptr[g0], w[g0:], mu, want_g=True)
    assert np.array_equal(_bits(part["group_norms"].cpu().numpy()), _bits(out["group_norms"].cpu().numpy()[g0:]))
    assert np.array_equal(_bits(part["g"].cpu().numpy()), _bits(out["g"].cpu().numpy()[r0:]))


def _cnorm_case(g, m, n, pool, ptr=None):
    from glx import kernels
    if ptr is None:
        ptr = gr.draw_groups(g, n, pool)
    w = g.uniform(0.5, 3.0, ptr.size - 1)
    A = g.standard_normal((m, n))
    want = gr.group_cnorms(A, ptr, w)
    cn, _ = kernels.col_norms(_dev(A))
    gcn, mx = kernels.group_cnorm(cn, ptr, w)
    got = gcn.cpu().numpy()
    max_run = int(np.diff(ptr).max())
    bar = ((m + 2) + (max_run + 3)) * gr.EPS64 / 2 * want
    err = np.abs(got.astype(LD) - want)
    assert np.all(err <= bar), (m, n, pool, float(np.max(err / bar)))
    assert mx.cpu().numpy()[0] == got.max()
    again, mx2 = kernels.group_cnorm(cn, ptr, w)
    assert np.array_equal(again.cpu().numpy(), got) and mx2.cpu().numpy()[0] == got.max()
    return cn, w, got


def test_group_cnorm():
    g = np.random.default_rng(3)
    for m, n, pool in ((96, 512, gr.POOL_SMALL), (96, 512, gr.POOL_LONG), (40, 130, gr.POOL_RAGGED), (5, 70, (1,)),
                       (7, 300, (300,))):
        _cnorm_case(g, m, n, pool)


# a lane per group (runs of at most 8: 262144 groups a trip) and a wave per group (4096 a trip), each
# 5 groups past one trip
@pytest.mark.parametrize("m,pool,G", [(3, (1, 2, 3), 262149), (5, (9, 10, 11, 12), 4101)], ids=["lane", "wave"])
def test_group_cnorm_several_trips(m, pool, G):
    from glx import kernels
    g = np.random.default_rng(5 + G)
    ptr = _draw_groups_at_once(g, G, pool)
    per_trip = 1024 * 256 // (1 if max(pool) <= 8 else 64)
    assert -(-G // per_trip) == 2 and np.diff(ptr).max() == max(pool)
    cn, w, got = _cnorm_case(g, m, int(ptr[-1]), pool, ptr=ptr)
    g0 = per_trip - 40          # the groups on both sides of the trip boundary, on their own: the same bits
    assert np.diff(ptr[g0:]).max() == max(pool)
    part, _ = kernels.group_cnorm(cn[int(ptr[g0]):].clone(), ptr[g0:] - ptr[g0], w[g0:])
    assert np.array_equal(_bits(part.cpu().numpy()), _bits(got[g0:]))


def _expand(kept, ptr, w, gcn, gmap=None):
    from glx import kernels
    G = ptr.size - 1
    K = len(kept)
    lst = np.full(max(64, (G + 63) // 64 * 64), -1, dtype=np.int32)
    lst[:K] = kept
    out = kernels.group_expand(_dev(lst), _dev(np.array([K, (K + 63) // 64 * 64], dtype=np.int32)), _dev(ptr),
                               _dev(w), _dev(gcn), None if gmap is None else _dev(gmap))
    rows, nptr, nw, ngcn, nmap, cnt = gr.expand_lists(kept, ptr, w, gcn, gmap)
    got = {key: v.cpu().numpy() for key, v in out.items()}
    assert list(got["count"]) == cnt
    assert np.array_equal(got["rows"][:cnt[1]], rows) and np.all(got["rows"][cnt[1]:] == -2)
    assert np.array_equal(got["group_ptr"][:K + 1], nptr) and np.all(got["group_ptr"][K + 1:] == -2)
    assert np.array_equal(got["weights"][:K], nw) and np.all(np.isnan(got["weights"][K:]))
    assert np.array_equal(got["gcn"][:K], ngcn) and np.all(np.isnan(got["gcn"][K:]))
    assert np.array_equal(got["map"][:K], nmap) and np.all(got["map"][K:] == -2)
    return nptr, nw, ngcn, nmap


@pytest.mark.parametrize("case", [(512, gr.POOL_SMALL), (512, gr.POOL_LONG), (130, gr.POOL_RAGGED), (700, (1,)),
                                  (5000, (1, 2, 3, 700))], ids=lambda c: "%d-%s" % (c[0], c[1][-1]))
def test_group_expand(case):
    n, pool = case
    g = np.random.default_rng(17 + n)
    _expand_case(g, gr.draw_groups(g, n, pool))


def test_group_expand_with_the_long_list_full():
    """More than 512 kept groups of more than 256 rows: the workgroup's LDS list of long groups
    fills up, and a thread that finds it full writes its group's rows itself. Which groups those
    are differs from run to run; the lists do not."""
    g = np.random.default_rng(23)
    sizes = g.choice([257, 258, 259, 260, 1, 2, 3], size=1101, p=[0.13, 0.13, 0.13, 0.13, 0.16, 0.16, 0.16])
    assert (sizes > 256).sum() >= 520
    _expand_case(g, np.concatenate(([0], np.cumsum(sizes))).astype(np.int32))


def _expand_case(g, ptr):
    G = ptr.size - 1
    assert G % 64 != 0
    w, gcn = g.uniform(0.5, 2.0, G), g.uniform(1.0, 9.0, G)
    lists = [np.arange(G), np.zeros(0, dtype=np.int64), np.array([int(g.integers(G))]), np.array([G - 1]),
             np.sort(g.choice(G, size=max(1, G // 3), replace=False))]
    for kept in lists:
        _expand(kept.astype(np.int32), ptr, w, gcn)
    # a second generation: the reduced description feeds the next expand, the map composes
    first = lists[-1].astype(np.int32)
    nptr, nw, ngcn, nmap = _expand(first, ptr, w, gcn)
    second = np.sort(g.choice(first.size, size=max(1, first.size // 2), replace=False)).astype(np.int32)
    _, _, _, m2 = _expand(second, nptr, nw, ngcn, nmap)
    assert np.array_equal(m2, first[second])


# ------------------------------------------------------------------------------------------ 3
@functools.lru_cache(maxsize=None)
def _solved(m, n, l, pool, ratio, screen, f32=False, tol=TOL):
    import glx
    ref = gr.reference_solution(m, n, l, pool, ratio, f32)
    dt = np.float32 if f32 else np.float64
    return glx.solve_certified(ref["A"].astype(dt), ref["b"].astype(dt), ref["mu"], tol=tol, screen=screen,
                               groups=ref["ptr"].copy(), weights=ref["w"].copy())


def _assert_safe(ref, info):
    G = ref["w"].size
    screened = np.ones(G, dtype=bool)
    screened[info["kept_groups"]] = False
    assert screened.sum() == G - len(info["kept_groups"])
    assert np.array_equal(info["kept_rows"], np.nonzero(gr.expand_rows(~screened, ref["ptr"]))[0])
    bad = np.nonzero(screened & ~(ref["gtheta"] < LD(ref["mu"])))[0]
    assert bad.size == 0, ("screened groups that are active at the reference solution", bad[:10])
    assert not np.any(screened & (gr.group_norms(ref["x"], ref["ptr"]) != 0))
    return screened


@pytest.mark.parametrize("case", gr.CASES, ids=lambda c: "%dx%dx%d-%s@%g" % (c[0], c[1], c[2], c[3][1], c[4]))
def test_group_certified_solve_f64(case):
    import glx
    m, n, l, pool, ratio = case
    ref = gr.reference_solution(m, n, l, pool, ratio)
    A, b, mu, ptr, w = ref["A"].copy(), ref["b"].copy(), ref["mu"], ref["ptr"].copy(), ref["w"].copy()
    x, info = _solved(m, n, l, pool, ratio, True)
    xu, infou = _solved(m, n, l, pool, ratio, False)
    print("\n%s: screened arm %d iterations, %d compactions %s, kept %d groups, width %d, passes %.1f, rel_gap %.2e; "
          "unscreened %d iterations, passes %.1f, rel_gap %.2e; reference rel_gap %.2e"
          % (case, info["iterations"], info["compactions"], info["kept_history"], info["kept"], info["width"],
             info["passes"], info["rel_gap"], infou["iterations"], infou["passes"], infou["rel_gap"],
             float(ref["gap"] / ref["primal"])))
    assert info["converged"] and infou["converged"]
    assert info["rel_gap"] <= TOL and infou["rel_gap"] <= TOL
    cert = glx.certificate(x, A, b, mu, ptr, w)
    assert set(cert) <= set(info) and "nonzero_rows" not in info
    for key in cert:
        if key != "plan":                     # (each entry describes its own kernels)
            assert info[key] == cert[key], key
    assert info["compactions"] >= 1 and info["width"] < n and info["kept"] < w.size
    assert info["kept_history"] == sorted(info["kept_history"], reverse=True)
    assert infou["compactions"] == 0 and infou["width"] == n
    assert np.array_equal(infou["kept_groups"], np.arange(w.size)) and np.array_equal(infou["kept_rows"], np.arange(n))
    assert info["passes"] < infou["passes"]
    _assert_safe(ref, info)
    P = float(ref["primal"])
    assert abs(info["primal"] - infou["primal"]) <= 2 * TOL * P
    from glx.certificate import _group_record, _inputs
    for xx, ii in ((x, info), (xu, infou)):
        rec = _group_record(*_inputs(xx, A, b), mu, (ptr, w), False)[0]
        slack = float(ref["gap"]) + gr.primal_bar(rec, mu, gr.EPS64, m, n, l, int(np.diff(ptr).max()), float(w.min()),
                                                  float(np.sum(A * A)), float(np.linalg.norm(b)))
        assert slack <= 1e-10 * P
        assert ii["primal"] >= float(ref["dual"]) - slack           # P(x) >= P* >= D_ref
        assert ii["primal"] - ii["gap"] <= P + slack                # D(theta) <= P* <= P_ref


def test_group_certified_solve_f32():
    m, n, l, pool, ratio = 96, 512, 16, gr.POOL_SMALL, 0.5
    ref = gr.reference_solution(m, n, l, pool, ratio, True)
    x, info = _solved(m, n, l, pool, ratio, True, True, 1e-4)
    print("\nf32: %d iterations, compactions %s, kept %d groups, rel_gap %.2e"
          % (info["iterations"], info["kept_history"], info["kept"], info["rel_gap"]))
    assert x.dtype == np.float32
    assert info["converged"]
    _assert_safe(ref, info)


# ------------------------------------------------------------------------------------------ 4
def test_single_row_groups_of_weight_one_are_the_row_path():
    import glx
    from glx.certificate import record
    m, n, l, ratio = 96, 512, 16, 0.1
    A, b, _, _ = gr.instance(gr.SEED, m, n, l, gr.POOL_SMALL)
    mu = ratio * glx.mu_max(A, b)
    ptr, ones = np.arange(n + 1, dtype=np.int32), np.ones(n)
    assert abs(glx.mu_max(A, b, ptr, ones) - glx.mu_max(A, b)) <= (l + 4) * gr.EPS64 * glx.mu_max(A, b)
    xr, ir = glx.solve_certified(A, b, mu, tol=TOL)
    xg, ig = glx.solve_certified(A, b, mu, tol=TOL, groups=ptr, weights=ones)
    assert ir["converged"] and ig["converged"]
    P = ir["primal"]
    assert abs(ig["primal"] - P) <= 2 * TOL * P
    assert np.array_equal(ig["kept_groups"], ig["kept_rows"])
    # the record of one iterate through both paths (fused = 2: the row kernel behind the same plain product)
    from glx.certificate import _group_record, _inputs
    u = gr.EPS64 / 2
    rrow = record(xg, A, b, mu, fused=2)
    rgrp, gq, _ = _group_record(*_inputs(xg, A, b), mu, (ptr, ones), True)
    gq = gq.cpu().numpy()
    gn = glx.certificate(xg, A, b, mu, fused=2, row_norms=True)["row_norms"]
    assert rgrp[0] == rrow[0] and rgrp[1] == rrow[1]           # the same two kernels
    e = 2 * (l / 2 + 2) * u
    assert np.all(np.abs(gq - gn) <= e * gn)
    assert abs(rgrp[3] - rrow[3]) <= e * rrow[3]
    assert abs(rgrp[2] - rrow[2]) <= (e + n * gr.EPS64) * rrow[2]
    B = 2 * (l / 2 + 5) * u * (gn + 2 * mu)
    assert abs(rgrp[4] - rrow[4]) <= B.max()
    kkt_i = gr.certificate(xg, A, b, mu, ptr, ones)["kkt"] + B     # (NumPy's, lifted to an upper bound per row)
    assert abs(rgrp[5] - rrow[5]) <= float(np.sum(2 * kkt_i * B + B * B)) + n * gr.EPS64 * rrow[5]
    assert rgrp[6] == rrow[6] and rgrp[7] == rrow[7] == 0.0


def test_weights_on_single_rows_are_a_column_scaling():
    import glx
    m, n, l, ratio = 96, 512, 16, 0.2
    A, b, _, _ = gr.instance(gr.SEED, m, n, l, gr.POOL_SMALL)
    w = np.random.default_rng(9).uniform(0.5, 2.0, n)
    mu = ratio * glx.mu_max(A, b, None, w)
    assert abs(glx.mu_max(A / w, b) - mu / ratio) <= 1e-12 * mu / ratio
    xw, iw = glx.solve_certified(A, b, mu, tol=TOL, weights=w)
    xs, isc = glx.solve_certified(A / w, b, mu, tol=TOL)
    assert iw["converged"] and isc["converged"]
    P = isc["primal"]
    assert abs(iw["primal"] - P) <= 2 * TOL * P
    # both are within their gaps of the optimum, and P(x) - P* >= 1/2 ||A (x - x*)||^2: the two images agree
    # to sqrt(2 gap) each (x itself is pinned only through A: m < n)
    img = np.linalg.norm(A @ xw - A @ (xs / w[:, None]))
    assert img <= np.sqrt(2 * iw["gap"]) + np.sqrt(2 * isc["gap"]) + 1e-12 * np.linalg.norm(b)
    assert set(np.nonzero(np.any(xw != 0, axis=1))[0]) <= set(iw["kept_rows"])


# ------------------------------------------------------------------------------------------ 5
def test_path_with_groups():
    import glx
    m, n, l = 96, 512, 16
    A, b, ptr, w = gr.instance(gr.SEED, m, n, l, gr.POOL_SMALL)
    tol = 1e-6
    out = glx.path(A, b, n_mus=4, mu_min_ratio=0.05, tol=tol, groups=ptr, weights=w)
    assert len(out) == 4
    mus = [o[0] for o in out]
    assert mus[0] == glx.mu_max(A, b, ptr, w) and mus[0] != glx.mu_max(A, b)
    assert abs(mus[0] - gr.mu_max(A, b, ptr, w)) <= 1e-12 * mus[0]
    mu0, x0, i0 = out[0]
    assert np.all(x0 == 0) and i0["iterations"] == 0 and i0["gap"] == 0.0 and i0["converged"]
    kept = [o[2]["kept"] for o in out]
    print("\npath: mu / mu_max %s, kept groups %s, iterations %s" % ([round(v / mus[0], 4) for v in mus], kept,
                                                                      [o[2]["iterations"] for o in out]))
    for mu, x, info in out:
        assert info["converged"] and info["rel_gap"] <= tol and info["mu"] == mu
        assert x.shape == (n, l) and "nonzero_groups" in info
    assert kept == sorted(kept)                     # non-increasing in mu


# ------------------------------------------------------------------------------------------ 6
def test_refusals_through_the_c_abi():
    from glx import _lib
    torch = _torch()
    h = _lib.lib()
    m, n, l = 40, 130, 3
    A, b, ptr, w = gr.instance(gr.SEED, m, n, l, gr.POOL_RAGGED)
    G = w.size
    Ad, bd = _dev(A), _dev(b)
    xd = torch.full((n, l), 3.25, dtype=torch.float64, device="cuda")
    nb = ctypes.c_size_t(0)
    _lib.check(h.glx_group_certified_workspace_bytes(_lib.GLX_F64, m, n, l, G, 1, ctypes.byref(nb)))
    ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    p = _lib.GlxProblem(dtype=_lib.GLX_F64, method=0, m=m, n=n, l=l, A=Ad.data_ptr(), b=bd.data_ptr(),
                        x=xd.data_ptr(), mu0=0.1, comm=None)

    def solve(pp, ww, wsb):
        info = _lib.GlxGroupCertifiedInfo()
        return h.glx_group_certified_solve(ctypes.byref(p), G, pp.ctypes.data, ww.ctypes.data, 1e-3, 1e-6, 10, 1, 10,
                                           None, None, None, None, ws.data_ptr(), wsb, ctypes.byref(info), None)

    bad_ptr = ptr.copy()
    bad_ptr[3] = bad_ptr[2]
    zero_w = w.copy()
    zero_w[G // 2] = 0.0
    for pp, ww, wsb, word in ((bad_ptr, w, ws.numel(), b"strictly increasing"), (ptr, zero_w, ws.numel(), b"weight"),
                              (ptr, w, ws.numel() - 256, b"workspace too small")):
        assert solve(pp, ww, wsb) == 1 and word in h.glx_last_error()
        torch.cuda.synchronize()
        assert torch.all(xd == 3.25).item() and torch.count_nonzero(ws).item() == 0   # nothing was launched
    rec = (ctypes.c_double * 8)()
    cb = ctypes.c_size_t(0)
    _lib.check(h.glx_group_certificate_workspace_bytes(_lib.GLX_F64, m, n, l, G, ctypes.byref(cb)))
    for pp, ww, wsb in ((bad_ptr, w, cb.value), (ptr, zero_w, cb.value), (ptr, w, cb.value - 256)):
        rc = h.glx_group_certificate(_lib.GLX_F64, m, n, l, Ad.data_ptr(), xd.data_ptr(), bd.data_ptr(), 0.1, G,
                                     pp.ctypes.data, ww.ctypes.data, None, None, rec, ws.data_ptr(), wsb, None)
        assert rc == 1
        torch.cuda.synchronize()
        assert torch.count_nonzero(ws).item() == 0
    p.comm = ws.data_ptr()
    assert solve(ptr, w, ws.numel()) == 1 and b"single-GPU" in h.glx_last_error()
