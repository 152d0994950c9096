"""The sparse-group lasso (DESIGN.md "Sparse-group lasso") in NumPy: the test reference.

    P(x) = 1/2 ||A x - b||_F^2 + mu Omega_tau(x),
    Omega_tau(x) = tau sum_i ||x_i||_2 + (1 - tau) sum_g w_g ||x_[g]||_F,   [g] = rows ptr[g] .. ptr[g + 1] - 1.

Write a = tau mu and c_g = (1 - tau) mu w_g. The dual is D(theta) = -1/2 ||theta||^2 - <theta, b> over
phi_g(1) <= c_g for every g, with rho_i = ||(A^T theta)_i|| and phi_g(s) = sqrt(sum_{i in g} (s rho_i - a)_+^2),
the norm of the row-wise shrinkage S_a of s (A^T theta)_[g]. phi_g is non-decreasing in s, so theta = s r with
s = min(1, min_g s_g), s_g = sup{s : phi_g(s) <= c_g}, is feasible. With R = sqrt(2 gap):

    row:    s rho_i + ||a_i|| R < a                      =>  x*_i = 0
    group:  phi_g(s) + ||A_[g]||_F R < c_g  (tau < 1)    =>  x*_[g] = 0

Holds Omega_tau, the two-level prox, k_sgl_fista's step in longdouble, the exact s_g by sorting, the
certificate and its KKT terms, both screening tests, the guard's mirror (glx_sgl_screen_guard, term by term),
k_sgl_expand's lists and a FISTA-with-screening reference with its cached high-accuracy solution. Reuses
group_ref's instance generator and pools. Imports nothing from glx.
"""
import functools

import numpy as np

import group_ref as gr

LD = gr.LD
EPS64 = gr.EPS64
EPS32 = gr.EPS32
TINY = gr.TINY
HALVINGS = 56   # k_sgl_dual_scale's trip count


def instance(seed, m, n, l, pool):
    """group_ref.instance's A, groups and weights with a truth that is sparse inside its groups: 10 % of the
    groups (at least one) are active, and an active group of more than one row has about half of its rows
    zero (never all). b = A u + 0.01 noise."""
    A, _, ptr, w = gr.instance(seed, m, n, l, pool)
    g = np.random.default_rng(seed + 1000)
    G = ptr.size - 1
    u = np.zeros((n, l))
    for k in g.choice(G, size=max(1, G // 10), replace=False):
        run = int(ptr[k + 1] - ptr[k])
        on = g.random(run) < 0.5
        on[g.integers(run)] = True
        u[ptr[k]:ptr[k + 1]] = g.standard_normal((run, l)) * on[:, None]
    b = A @ u + 0.01 * g.standard_normal((m, l))
    return A, b, ptr, w


def row_norms(v):
    return np.sqrt(np.sum(v * v, axis=1))


def omega(x, ptr, w, tau):
    """Omega_tau(x) in x's dtype."""
    wide = x.dtype.type
    return wide(tau) * np.sum(row_norms(x)) + wide(1 - tau) * np.sum(np.asarray(w).astype(wide) * gr.group_norms(x, ptr))


def prox(wv, ta, tcw, ptr):
    """argmin_x 1/2 ||x - wv||^2 + ta sum_i ||x_i|| + sum_g tcw_g ||x_[g]||: the row shrinkage, then the
    group shrinkage of its result (q_g = ||u_[g]||_F = sqrt(sum (||w_i|| - ta)_+^2))."""
    rho = row_norms(wv)
    c1 = np.maximum(rho - ta, 0)
    u = wv * (c1 / np.where(rho > 0, rho, 1))[:, None]
    q = np.sqrt(np.add.reduceat(c1 * c1, np.asarray(ptr[:-1], dtype=np.intp)))
    sc = np.where(q > tcw, 1 - tcw / np.where(q > 0, q, 1), 0)
    return u * gr.expand_rows(sc, ptr)[:, None]


def step_ref(y, g, xk, ptr, w, t, mu, tau, thres, theta, theta_next):
    """k_sgl_fista's step in longdouble, from inputs given in the working dtype T: the scalars are rounded to
    T first, as the kernel does (t a and t (1 - tau) mu are double products rounded to T). Returns (xc,
    v_next, y_next, sums, rho = ||w_i||, q_g, t a, t c_g)."""
    T = y.dtype.type
    tl, thl, a1, b1 = LD(T(t)), LD(T(theta)), LD(T(1.0 - theta_next)), LD(T(theta_next))
    ta = LD(T(float(t) * (float(tau) * float(mu))))
    wT = np.asarray(w).astype(T).astype(LD)
    tcw = LD(T(float(t) * ((1.0 - float(tau)) * float(mu)))) * wT
    yl, gl, xl = y.astype(LD), g.astype(LD), xk.astype(LD)
    wv = yl - tl * gl
    rho = row_norms(wv)
    c1 = np.maximum(rho - ta, 0)
    d1 = (rho < LD(thres)).astype(LD) + rho
    q = np.sqrt(np.add.reduceat(c1 * c1, np.asarray(ptr[:-1], dtype=np.intp)))
    c2 = np.maximum(q - tcw, 0)
    d2 = (q < LD(thres)).astype(LD) + q
    xc = wv * (c1 / d1)[:, None] * gr.expand_rows(c2 / d2, ptr)[:, None]
    xo = np.where(np.abs(xl) < LD(thres), 0, xl)
    vn = xo + (xc - xo) / thl
    yn = a1 * np.where(np.abs(xc) < LD(thres), 0, xc) + b1 * vn
    pen = LD(T(tau)) * np.sum(row_norms(xc)) + LD(T(1.0 - tau)) * np.sum(wT * gr.group_norms(xc, ptr))
    sums = [np.sum(gl * (xc - yl)), np.sum((xc - yl) ** 2), pen, np.max(np.abs(xc))]
    return xc, vn, yn, sums, rho, q, ta, tcw


def phi(s, rho, a):
    """phi(s) of one group's row norms, in their dtype."""
    v = np.maximum(s * rho - a, 0)
    return np.sqrt(np.sum(v * v))


def exact_s(rho, a, c):
    """sup{s >= 0 : phi(s) <= c} of one group in longdouble, by sorting: phi vanishes up to a / max rho and
    its active set between the breakpoints a / rho_(k), a / rho_(k+1) is the k largest rows, where
    phi(s) = c is a quadratic in s. +inf where every rho is 0; a / max rho where c = 0."""
    r = np.sort(np.asarray(rho, dtype=LD))[::-1]
    a, c = LD(a), LD(c)
    r = r[r > 0]
    if r.size == 0:
        return LD(np.inf)
    if c == 0:
        return a / r[0]
    k = 1
    for j in range(1, r.size):   # the largest k with phi(a / rho_(k)) <= c (phi(a / rho_(1)) = 0)
        if phi(a / r[j], r, a) <= c:
            k = j + 1
        else:
            break
    p1, p2 = np.sum(r[:k]), np.sum(r[:k] * r[:k])
    disc = a * a * p1 * p1 - p2 * (LD(k) * a * a - c * c)
    return (a * p1 + np.sqrt(max(disc, LD(0)))) / p2


def exact_sg(rho, ptr, w, a, cb):
    """exact_s for every group, c_g = cb w_g: longdouble array of G."""
    return np.array([exact_s(rho[ptr[k]:ptr[k + 1]], a, LD(cb) * LD(w[k])) for k in range(len(ptr) - 1)], dtype=LD)


def halving_bound(rho, ptr, w, a, cb):
    """How far below the exact s_g the kernel's value may lie by its termination rule: the bracket
    [0, (a + c_g) / max rho] after HALVINGS halvings, per group (0 where c_g = 0 or the group is all zero)."""
    out = np.zeros(len(ptr) - 1, dtype=LD)
    for k in range(len(ptr) - 1):
        pm = np.max(rho[ptr[k]:ptr[k + 1]])
        c = LD(cb) * LD(w[k])
        if pm > 0 and c > 0:
            out[k] = (LD(a) + c) / LD(pm) * LD(2.0) ** (-HALVINGS)
    return out


def kkt_terms(x, g, mu, ptr, w, tau):
    """The distances from -g to mu dOmega_tau(x), one per row of a nonzero group and one per zero group, in
    the arrays' dtype: (terms of the rows (0 where the row's group is zero), terms of the groups (0 where
    nonzero))."""
    wide = x.dtype.type
    a = wide(tau) * wide(mu)
    cg = wide(1 - tau) * wide(mu) * np.asarray(w).astype(wide)
    rho, xn = row_norms(g), row_norms(x)
    xg = gr.group_norms(x, ptr)
    nzg = gr.expand_rows(xg != 0, ptr)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = g + (a / np.where(xn != 0, xn, 1))[:, None] * x + gr.expand_rows(cg / np.where(xg != 0, xg, 1), ptr)[:, None] * x
    d = np.maximum(rho - a, 0)
    rows = np.where(nzg, np.where(xn != 0, row_norms(k), d), 0)
    ph = np.sqrt(np.add.reduceat(d * d, np.asarray(ptr[:-1], dtype=np.intp)))
    groups = np.where(xg != 0, 0, np.maximum(ph - cg, 0))
    return rows, groups


def cert_terms(x, g, mu, ptr, w, tau):
    """k_sgl_cert's six sums and the row norms from a given g, in the arrays' dtype."""
    rows, groups = kkt_terms(x, g, mu, ptr, w, tau)
    rho = row_norms(g)
    return {"row_norms": rho, "sums": [omega(x, ptr, w, tau), np.max(rho), max(np.max(rows), np.max(groups)),
                                       np.sum(rows * rows) + np.sum(groups * groups),
                                       float(np.sum(gr.group_norms(x, ptr) != 0)), float(np.sum(row_norms(x) != 0))]}


def certificate(x, A, b, mu, ptr, w, tau):
    """The sparse-group certificate in the arrays' dtype (pass longdouble arrays for a reference)."""
    wide = x.dtype.type
    r = A @ x - b
    g = A.T @ r
    c = cert_terms(x, g, mu, ptr, w, tau)
    sg = exact_sg(c["row_norms"], ptr, w, LD(tau) * LD(mu), LD(1 - tau) * LD(mu))
    smin = np.min(sg)
    s = wide(min(smin, LD(1)))
    rr, rb, om = np.sum(r * r), np.sum(r * b), c["sums"][0]
    primal = rr / 2 + wide(mu) * om
    dual = -s * s * rr / 2 - s * rb
    return {"r": r, "g": g, "row_norms": c["row_norms"], "rr": rr, "rb": rb, "omega": om, "s_g": sg, "s_min": smin,
            "scale": s, "primal": primal, "dual": dual, "gap": primal - dual,
            "rel_gap": (primal - dual) / max(abs(primal), wide(TINY)), "kkt_max": c["sums"][2], "kkt_sq": c["sums"][3],
            "nonzero_groups": int(c["sums"][4]), "nonzero_rows": int(c["sums"][5])}


def mu_max(A, b, ptr, w, tau):
    """The smallest mu at which x = 0 is optimal: 1 / min_g s_g of g = A^T b at mu = 1."""
    rho = row_norms((A.T @ b).astype(LD))
    return float(1 / np.min(exact_sg(rho, ptr, w, LD(tau), LD(1 - tau))))


def keep_rows(rho, cn, gcn, ptr, w, s, mul, add, rad, a_lo, cb_lo, group_test=True):
    """Both tests in longdouble on p_i = mul rho_i + add: (row flags, group flags); True = kept."""
    p = LD(mul) * rho.astype(LD) + LD(add)
    with np.errstate(invalid="ignore"):
        rgone = LD(s) * p + cn.astype(LD) * LD(rad) < LD(a_lo)
        v = np.maximum(LD(s) * p - LD(a_lo), 0)
        ph = np.sqrt(np.add.reduceat(v * v, np.asarray(ptr[:-1], dtype=np.intp)))
        ggone = (ph / np.asarray(w).astype(LD) + gcn.astype(LD) * LD(rad) < LD(cb_lo)) & bool(group_test)
    keep = ~rgone & ~gr.expand_rows(ggone, ptr)
    return keep, np.add.reduceat(keep.astype(np.int64), np.asarray(ptr[:-1], dtype=np.intp)) > 0


def guard_pad(eps, m, l, max_run, cmax, weighted=False):
    """(mul, add coefficient) of glx_sgl_screen_guard: mul rho^_i + add ||r^|| >= ||a_i^T r^|| for every row."""
    k = 3.0 if weighted else 2.0
    gm, gl = gr.gamma(m + k, eps), gr.gamma(l + 2.0, eps)
    ev = 1.0 + gr.gamma(max_run + 16.0, EPS64)
    g_ml = gr.gamma(float(m) * float(l) + k, EPS64)
    return (1.0 + gl) * ev, gm * cmax * (1.0 + gr.gamma(m + k, EPS64)) * (1.0 + g_ml) * ev * (1.0 + 4.0 * EPS64)


def guard(rec, s_pad, mu, tau, eps, m, n, l, max_run, w_min, cmax, col_sumsq, b_norm, weighted=False):
    """(mul, add, s_safe, gap+, rho+): glx_sgl_screen_guard in float64, term by term (the module docstring of
    group_ref.guard, with the padding in place of its items 1 and 3)."""
    k = 3.0 if weighted else 2.0
    rr, rb, om = (float(v) for v in rec[:3])
    rn = np.sqrt(rr)
    gn = gr.gamma(n + 2.0, eps)
    gK = gr.gamma(float(max_run) * float(l) + 4.0, eps)
    g_ml = gr.gamma(float(m) * float(l) + k, EPS64)
    bn = b_norm * (1.0 + g_ml) if weighted else b_norm
    up = (1.0 + gr.gamma(m + k, EPS64)) * (1.0 + gr.gamma(max_run + 3.0, EPS64))
    mul, addc = guard_pad(eps, m, l, max_run, cmax, weighted)
    s = s_pad if s_pad < 1.0 else (1.0 if s_pad >= 1.0 else s_pad)
    wq = tau + (1.0 - tau) * w_min
    dr = gn * np.sqrt(col_sumsq) * (om / wq) + eps * (rn + 2.0 * bn)
    bar_rr = g_ml * rr
    bar_rb = g_ml * rn * bn
    bar_sx = (gK + gr.gamma(2.0 * n + 2.0, EPS64)) * om
    gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * om
    bars = rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx
    gap_p = (gap if gap > 0.0 else (0.0 if gap <= 0.0 else gap)) + bars
    return float(mul), float(addc * rn), float(s), float(gap_p), float(np.sqrt(2.0 * gap_p) * up)


def expand_lists(keep, ptr, w, gcn, gmap=None):
    """k_sgl_expand in NumPy: (rows padded with -1 to a multiple of 64, new group_ptr over the groups that
    keep a row, their weights, gcn (carried over), composed map, [groups, rows, rows, padded rows])."""
    keep = np.asarray(keep).astype(bool)
    rows = np.flatnonzero(keep)
    per = np.add.reduceat(keep.astype(np.int64), np.asarray(ptr[:-1], dtype=np.intp))
    alive = np.flatnonzero(per > 0)
    wp = (rows.size + 63) // 64 * 64
    padded = np.concatenate((rows, -np.ones(wp - rows.size, dtype=np.int64))).astype(np.int32)
    nptr = np.concatenate(([0], np.cumsum(per[alive]))).astype(np.int32)
    gm = alive if gmap is None else np.asarray(gmap)[alive]
    return padded, nptr, np.asarray(w)[alive], np.asarray(gcn)[alive], gm.astype(np.int32), [alive.size, rows.size,
                                                                                          rows.size, wp]


def fista_screen(A, b, mu, ptr, w, tau, tol=1e-8, maxit=400000, screen=True, check_every=10):
    """FISTA with the two-level prox, the step 1 / lambda_max(A^T A), adaptive restart and the two gap-safe
    tests (the plain ones, in float64) on the columns still kept. Returns (x, info): info["kept_rows"] = bool
    mask over rows, "kept_row_history" = kept rows after each reduction."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    n = A.shape[1]
    l = b.shape[1]
    t = 1.0 / float(np.linalg.eigvalsh(A.T @ A)[-1])
    w = np.asarray(w, dtype=np.float64)
    cn_all = np.sqrt(np.sum(A * A, axis=0))
    rows = np.arange(n)
    Ac, pc, wc = A, np.asarray(ptr), w
    x = np.zeros((n, l))
    y = x.copy()
    k, it, rel = 1, 0, np.inf
    hist = []
    while True:
        if it % check_every == 0 or it >= maxit:
            c = certificate(x, Ac, b, mu, pc, wc, tau)
            rel = float(c["rel_gap"])
            if rel <= tol or it >= maxit:
                break
            if screen:
                cn = cn_all[rows]
                gcn = np.sqrt(np.add.reduceat(cn * cn, np.asarray(pc[:-1], dtype=np.intp))) / wc
                rad = np.sqrt(2.0 * max(float(c["gap"]), 0.0)) * (1.0 + 1e-9)
                keep, _ = keep_rows(c["row_norms"], cn, gcn, pc, wc, float(c["scale"]) * (1.0 - 1e-12), 1.0, 0.0, rad,
                                    tau * mu, (1.0 - tau) * mu, tau < 1.0)
                if not keep.all():
                    per = np.add.reduceat(keep.astype(np.int64), np.asarray(pc[:-1], dtype=np.intp))
                    alive = per > 0
                    pc = np.concatenate(([0], np.cumsum(per[alive])))
                    wc, rows, Ac, x = wc[alive], rows[keep], Ac[:, keep], x[keep]
                    y, k = x.copy(), 1
                    hist.append(int(keep.sum()))
                    if rows.size == 0:
                        break
        theta, theta_next = 2.0 / (k + 1), 2.0 / (k + 2)
        g = Ac.T @ (Ac @ y - b)
        xc = prox(y - t * g, t * tau * mu, t * (1.0 - tau) * mu * wc, pc)
        if float(np.sum((y - xc) * (xc - x))) > 0.0:
            y, k = xc.copy(), 1
        else:
            v = x + (xc - x) / theta
            y = (1.0 - theta_next) * xc + theta_next * v
            k += 1
        x = xc
        it += 1
    full = np.zeros((n, l))
    full[rows] = x
    kept = np.zeros(n, dtype=bool)
    kept[rows] = True
    return full, {"iterations": it, "kept_rows": kept, "rel_gap": rel, "kept_row_history": hist}


SEED = 1
# (m, n, l, pool, tau, ratio of mu_max)
CASES = [(96, 512, 16, gr.POOL_SMALL, 0.3, 0.3), (96, 512, 16, gr.POOL_LONG, 0.9, 0.3),
         (40, 130, 3, gr.POOL_RAGGED, 0.3, 0.2), (40, 130, 3, gr.POOL_RAGGED, 1.0, 0.2)]


@functools.lru_cache(maxsize=None)
def reference_solution(m, n, l, pool, tau, ratio, f32=False):
    """:func:`instance` (seed SEED) at mu = ratio * mu_max(tau) and its reference solution: float64 FISTA
    with restarts and screening down to the float64 gap's floor, then the certificate of the result in
    longdouble, which must show rel_gap <= 1e-11. Returns a dict: A, b, ptr, w, tau, mu, x (float64), primal,
    dual, gap (longdouble), support (bool mask over rows). Shared: do not modify."""
    A, b, ptr, w = instance(SEED, m, n, l, pool)
    if f32:
        A, b = A.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
        w = w.astype(np.float32).astype(np.float64)
    mu = float(ratio) * mu_max(A, b, ptr, w, tau)
    x, info = fista_screen(A, b, mu, ptr, w, tau, tol=2e-14)
    c = certificate(x.astype(LD), A.astype(LD), b.astype(LD), LD(mu), ptr, w, tau)
    assert float(c["rel_gap"]) <= 1e-11, ("the reference did not reach 1e-11", float(c["rel_gap"]), info)
    for arr in (A, b, x, ptr, w):
        arr.setflags(write=False)
    return {"A": A, "b": b, "ptr": ptr, "w": w, "tau": tau, "mu": mu, "x": x, "primal": c["primal"], "dual": c["dual"],
            "gap": c["gap"], "support": row_norms(x) != 0, "iterations": info["iterations"]}
