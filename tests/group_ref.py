"""Feature groups and weights (DESIGN.md "Feature groups and weights") in NumPy: the test reference.

    P(x) = 1/2 ||A x - b||_F^2 + mu sum_g w_g ||x_[g]||_F,   [g] = rows ptr[g] .. ptr[g + 1] - 1,

with the dual D(theta) = -1/2 ||theta||^2 - <theta, b> over ||A_[g]^T theta||_F <= mu w_g. As for rows,
theta* = A x* - b and a dual-feasible theta has ||theta - theta*|| <= sqrt(2 gap), so

    s ||g_[g]|| / w_g + (||A_[g]||_F / w_g) rho < mu,  theta = s r, g = A^T r, rho = sqrt(2 gap)  =>  x*_[g] = 0

(||A_[g]||_2 <= ||A_[g]||_F). Holds the seeded instance generator, the group certificate in any
precision, the rounding guard's formulae (the mirror of glx_group_screen_guard, term by term), the
FISTA step of k_group_fista in longdouble, k_group_expand's lists, and a FISTA-with-screening
reference with its cached high-accuracy solution. Imports nothing from glx.
"""
import functools

import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
TINY = float(np.finfo(np.float64).tiny)

POOL_SMALL = (1, 2, 3, 5, 8)
POOL_LONG = (1, 64, 65, 7)
POOL_RAGGED = (1, 2, 3, 5)


def draw_groups(g, n, pool):
    """Sizes drawn from `pool` until they sum to n (the last one cut to fit): group_ptr, int32."""
    sizes = []
    left = int(n)
    while left > 0:
        s = min(int(g.choice(pool)), left)
        sizes.append(s)
        left -= s
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)


def instance(seed, m, n, l, pool):
    """The issue's generator: (A, b, group_ptr, weights = sqrt(size)), float64. The truth has 10 % of
    the groups (at least one) active with normal entries; b = A u + 0.01 noise."""
    g = np.random.default_rng(seed)
    ptr = draw_groups(g, n, pool)
    G = ptr.size - 1
    A = g.standard_normal((m, n))
    u = np.zeros((n, l))
    for k in g.choice(G, size=max(1, G // 10), replace=False):
        u[ptr[k]:ptr[k + 1]] = g.standard_normal((ptr[k + 1] - ptr[k], l))
    b = A @ u + 0.01 * g.standard_normal((m, l))
    return A, b, ptr, np.sqrt(np.diff(ptr).astype(np.float64))


def group_norms(v, ptr):
    """||v_[g]||_F for every group of the (n x l) array v, in v's dtype."""
    sq = np.sum(v * v, axis=1)
    return np.sqrt(np.add.reduceat(sq, np.asarray(ptr[:-1], dtype=np.intp)))


def expand_rows(per_group, ptr):
    return np.repeat(per_group, np.diff(ptr))


def mu_max(A, b, ptr, w):
    return float(np.max(group_norms(A.T @ b, ptr) / w))


def certificate(x, A, b, mu, ptr, w):
    """The group certificate in the arrays' dtype (pass longdouble arrays for a reference)."""
    wide = x.dtype.type
    w = np.asarray(w).astype(wide)
    r = A @ x - b
    g = A.T @ r
    gn, xn = group_norms(g, ptr), group_norms(x, ptr)
    gq = gn / w
    nz = xn != 0
    muw = wide(mu) * w
    with np.errstate(invalid="ignore", divide="ignore"):
        k = g + expand_rows(np.where(nz, muw / np.where(nz, xn, 1), 0), ptr)[:, None] * x
    kkt = np.where(nz, group_norms(k, ptr), np.maximum(gn - muw, 0))
    rr, rb, sxw, gmax = np.sum(r * r), np.sum(r * b), np.sum(w * xn), np.max(gq)
    s = wide(1) if gmax <= mu else wide(mu) / gmax
    primal = rr / 2 + wide(mu) * sxw
    dual = -s * s * rr / 2 - s * rb
    return {"r": r, "g": g, "group_norms": gq, "rr": rr, "rb": rb, "sum_xnorm": sxw, "gmax": gmax, "scale": s,
            "primal": primal, "dual": dual, "gap": primal - dual,
            "rel_gap": (primal - dual) / max(abs(primal), wide(TINY)), "kkt": kkt, "kkt_max": np.max(kkt),
            "kkt_sq": np.sum(kkt * kkt), "nonzero_groups": int(np.sum(nz))}


def record(cert):
    return [float(cert["rr"]), float(cert["rb"]), float(cert["sum_xnorm"]), float(cert["gmax"]),
            float(cert["kkt_max"]), float(cert["kkt_sq"]), float(cert["nonzero_groups"]), 0.0]


def gamma(k, u):
    ku = float(k) * u
    return ku / (1.0 - ku) if ku < 1.0 else float("inf")


def group_cnorms(A, ptr, w, wide=LD):
    """gcn[g] = ||A_[g]||_F / w_g in `wide`."""
    a = A.astype(wide)
    return np.sqrt(np.add.reduceat(np.sum(a * a, axis=0), np.asarray(ptr[:-1], dtype=np.intp))) / np.asarray(w).astype(wide)


def guard(rec, mu, eps, m, n, l, max_run, w_min, gcol_max, col_sumsq, b_norm):
    """(s_safe, gap+, rho+): glx_group_screen_guard in float64, term by term. K = max_run l terms in a
    group's norm; gK = gamma_{K+3}(eps) is that norm in A's dtype plus the weight's one rounding; `up`
    lifts the stored gcn (the column norms' gamma64_{m+2}, then a root of <= max_run doubles and a
    division: gamma64_{max_run+3}).
      1. s_safe = min(1, mu / (gmax (1 + gK) + gamma_m gcol_max up ||r||));
      2. ||x||_F <= rec[2] / w_min in delta_r; sum_g w_g ||x_[g]|| carries gK + gamma64_{n+2};
      3. rho+ = (sqrt(2 gap+) + s gamma_m ||r|| + s gK (1 + gamma_m) ||r||) up."""
    rr, rb, sxw, gmax = (float(v) for v in rec[:4])
    rn = np.sqrt(rr)
    gm, gn = gamma(m + 2, eps), gamma(n + 2, eps)
    gK = gamma(float(max_run) * float(l) + 3.0, eps)
    up = (1.0 + gamma(m + 2, EPS64)) * (1.0 + gamma(max_run + 3, EPS64))
    den = gmax * (1.0 + gK) + gm * gcol_max * up * rn
    s = mu / den if den > mu else (1.0 if den <= mu else den)
    dr = gn * np.sqrt(col_sumsq) * (sxw / w_min) + eps * (rn + 2.0 * b_norm)
    g_ml = gamma(float(m) * float(l) + 2.0, EPS64)
    bar_rr = g_ml * rr
    bar_rb = g_ml * rn * b_norm
    bar_sx = (gK + gamma(n + 2, EPS64)) * sxw
    gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * sxw
    bars = rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx
    gap_p = (gap if gap > 0.0 else (0.0 if gap <= 0.0 else gap)) + bars
    rho = np.sqrt(2.0 * gap_p) + s * gm * rn + s * gK * (1.0 + gm) * rn
    rho *= up
    return float(s), float(gap_p), float(rho)


def primal_bar(rec, mu, eps, m, n, l, max_run, w_min, col_sumsq, b_norm):
    """How far the primal value composed from the record can be from P(x): the guard's item 2 with
    its sums' bars (the dual's terms left out)."""
    rr, _, sxw = (float(v) for v in rec[:3])
    rn = np.sqrt(rr)
    dr = gamma(n + 2, eps) * np.sqrt(col_sumsq) * (sxw / w_min) + eps * (rn + 2.0 * b_norm)
    bar_rr = gamma(float(m) * float(l) + 2.0, EPS64) * rr
    bar_sx = (gamma(float(max_run) * float(l) + 3.0, eps) + gamma(n + 2, EPS64)) * sxw
    return float(rn * dr + 0.5 * dr * dr + 0.5 * bar_rr + mu * bar_sx)


def keep_mask(gq, gcn, s, rho, mu):
    """The test in longdouble: True = kept."""
    lhs = LD(s) * gq.astype(LD) + gcn.astype(LD) * LD(rho)
    with np.errstate(invalid="ignore"):
        return ~(lhs < LD(mu))


def prox(wv, tmuw, ptr):
    """The group prox: tmuw = t mu w_g per group."""
    nrm = group_norms(wv, ptr)
    scale = np.where(nrm > tmuw, 1 - tmuw / np.where(nrm > 0, nrm, 1), 0)
    return wv * expand_rows(scale, ptr)[:, None]


def step_ref(y, g, xk, ptr, w, t, mu, thres, theta, theta_next):
    """k_group_fista's step in longdouble, from inputs given in the working dtype T: t, mu, w_g and
    the momentum scalars are rounded to T first, as the kernel does, and t mu is the double product
    rounded to T. Returns (xc, v_next, y_next, sums, ||w_[g]||, t mu w_g)."""
    T = y.dtype.type
    tl, thl, a1, b1 = LD(T(t)), LD(T(theta)), LD(T(1.0 - theta_next)), LD(T(theta_next))
    tmuw = LD(T(float(t) * float(mu))) * np.asarray(w).astype(T).astype(LD)
    yl, gl, xl = y.astype(LD), g.astype(LD), xk.astype(LD)
    wv = yl - tl * gl
    nrm = group_norms(wv, ptr)
    c = np.maximum(nrm - tmuw, 0)
    d = (nrm < LD(thres)).astype(LD) + nrm
    xc = wv * expand_rows(c / d, ptr)[:, None]
    xo = np.where(np.abs(xl) < LD(thres), 0, xl)
    vn = xo + (xc - xo) / thl
    yn = a1 * np.where(np.abs(xc) < LD(thres), 0, xc) + b1 * vn
    sums = [np.sum(gl * (xc - yl)), np.sum((xc - yl) ** 2),
            np.sum(np.asarray(w).astype(T).astype(LD) * group_norms(xc, ptr)), np.max(np.abs(xc))]
    return xc, vn, yn, sums, nrm, tmuw


def expand_lists(kept, ptr, w, gcn, gmap=None):
    """k_group_expand in NumPy: (rows padded with -1 to a multiple of 64, new group_ptr, weights, gcn,
    composed map, [rows, padded rows])."""
    kept = np.asarray(kept, dtype=np.int64)
    rows = np.concatenate([np.arange(ptr[k], ptr[k + 1]) for k in kept]) if kept.size else np.zeros(0, np.int64)
    wp = (rows.size + 63) // 64 * 64
    padded = np.concatenate((rows, -np.ones(wp - rows.size, dtype=np.int64))).astype(np.int32)
    nptr = np.concatenate(([0], np.cumsum(np.diff(ptr)[kept]))).astype(np.int32)
    gm = kept if gmap is None else np.asarray(gmap)[kept]
    return padded, nptr, np.asarray(w)[kept], np.asarray(gcn)[kept], gm.astype(np.int32), [rows.size, wp]


def fista_screen(A, b, mu, ptr, w, tol=1e-8, maxit=400000, screen=True, check_every=10, use_guard=True):
    """FISTA with the group prox, the step 1 / lambda_max(A^T A), adaptive restart and gap-safe
    screening on groups, in float64 on the columns still kept. use_guard=False is the issue's model
    (the plain Frobenius-norm test). Returns (x, info): info["kept"] = bool mask over groups,
    "kept_history" = kept rows after each reduction, "widths" = their padded widths."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    m, n = A.shape
    l = b.shape[1]
    t = 1.0 / float(np.linalg.eigvalsh(A.T @ A)[-1])
    w = np.asarray(w, dtype=np.float64)
    gcn_all = np.asarray(group_cnorms(A, ptr, w), dtype=np.float64)
    csq, bn = float(np.sum(A * A)), float(np.linalg.norm(b))
    max_run, w_min, gcmax = int(np.diff(ptr).max()), float(w.min()), float(gcn_all.max())
    gidx = np.arange(ptr.size - 1)
    rows = np.arange(n)
    Ac, pc, wc = A, np.asarray(ptr), w
    x = np.zeros((n, l))
    y = x.copy()
    k, it, rel = 1, 0, np.inf
    hist, widths = [], []
    while True:
        if it % check_every == 0 or it >= maxit:
            c = certificate(x, Ac, b, mu, pc, wc)
            rel = float(c["rel_gap"])
            if rel <= tol or it >= maxit:
                break
            if screen:
                if use_guard:
                    s, _, rho = guard(record(c), mu, EPS64, m, Ac.shape[1], l, max_run, w_min, gcmax, csq, bn)
                    keep = keep_mask(c["group_norms"], gcn_all[gidx], s, rho, mu * (1.0 - 4.0 * EPS64))
                else:
                    keep = keep_mask(c["group_norms"], gcn_all[gidx], float(c["scale"]),
                                     np.sqrt(2.0 * max(float(c["gap"]), 0.0)), mu)
                if not keep.all():
                    rk = expand_rows(keep, pc)
                    pc = np.concatenate(([0], np.cumsum(np.diff(pc)[keep])))
                    gidx, wc, rows, Ac, x = gidx[keep], wc[keep], rows[rk], Ac[:, rk], x[rk]
                    y, k = x.copy(), 1
                    hist.append(int(rk.sum()))
                    widths.append((int(rk.sum()) + 63) // 64 * 64)
                    if gidx.size == 0:
                        break
        theta, theta_next = 2.0 / (k + 1), 2.0 / (k + 2)
        g = Ac.T @ (Ac @ y - b)
        xc = prox(y - t * g, t * mu * wc, pc)
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
    kept = np.zeros(ptr.size - 1, dtype=bool)
    kept[gidx] = True
    return full, {"iterations": it, "kept": kept, "rel_gap": rel, "kept_history": hist, "widths": widths}


SEED = 1
CASES = [(96, 512, 16, POOL_SMALL, 0.5), (96, 512, 16, POOL_SMALL, 0.1), (96, 512, 16, POOL_LONG, 0.5),
         (96, 512, 16, POOL_LONG, 0.1), (40, 130, 3, POOL_RAGGED, 0.1)]


@functools.lru_cache(maxsize=None)
def reference_solution(m, n, l, pool, ratio, f32=False):
    """The instance (seed SEED) at mu = ratio * mu_max and its reference solution: float64 FISTA with
    restarts and guarded screening down to the float64 gap's floor, then the certificate of the
    result in longdouble, which must show rel_gap <= 1e-12. Returns a dict: A, b, ptr, w, mu, x
    (float64), theta (longdouble A x - b), gtheta (longdouble ||A_[g]^T theta|| / w_g), primal, dual,
    gap (longdouble). f32: A and b rounded to float32 first (w too). Shared: do not modify."""
    A, b, ptr, w = instance(SEED, m, n, l, pool)
    if f32:
        A, b = A.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
        w = w.astype(np.float32).astype(np.float64)
    mu = float(ratio) * mu_max(A, b, ptr, w)
    x, info = fista_screen(A, b, mu, ptr, w, tol=2e-14)
    c = certificate(x.astype(LD), A.astype(LD), b.astype(LD), LD(mu), ptr, w)
    assert float(c["rel_gap"]) <= 1e-12, ("the reference did not reach 1e-12", float(c["rel_gap"]), info)
    for a in (A, b, x, ptr, w):
        a.setflags(write=False)
    return {"A": A, "b": b, "ptr": ptr, "w": w, "mu": mu, "x": x, "theta": c["r"], "gtheta": c["group_norms"],
            "primal": c["primal"], "dual": c["dual"], "gap": c["gap"], "iterations": info["iterations"]}
