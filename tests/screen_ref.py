"""Gap-safe screening (DESIGN.md "Certified solve and screening") in NumPy: the test reference.

For P(x) = 1/2 ||A x - b||_F^2 + mu sum_i ||x_i||_2 and its dual D(theta) = -1/2 ||theta||^2 -
<theta, b> over ||a_i^T theta|| <= mu (a_i = column i of A): theta* = A x* - b, D is 1-strongly
concave, so a dual-feasible theta has ||theta - theta*|| <= sqrt(2 gap), and

    s ||g_i|| + ||a_i|| rho < mu  with  theta = s r, g = A^T r, rho = sqrt(2 gap)   =>   x*_i = 0.

Holds the column norms, the unguarded test in np.longdouble, the rounding guard's formulae (the
mirror of glx_screen_guard, term by term), a FISTA-with-screening reference and the high-accuracy
reference solution the safety tests compare with. Imports nothing from glx except, through
certificate_ref, the instance generator.
"""
import functools

import numpy as np

import certificate_ref as cref

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)


def col_norms(A, wide=LD):
    """||a_i||_2 of every column, in `wide`."""
    a = A.astype(wide)
    return np.sqrt(np.sum(a * a, axis=0))


def keep_mask(row_norms, cn, s, rho, mu):
    """The unguarded test in longdouble: True = kept (the test does not hold strictly, or a NaN)."""
    lhs = LD(s) * row_norms.astype(LD) + cn.astype(LD) * LD(rho)
    with np.errstate(invalid="ignore"):
        return ~(lhs < LD(mu))


def gamma(k, u):
    ku = float(k) * u
    return ku / (1.0 - ku) if ku < 1.0 else float("inf")


def guard(rec, mu, eps, m, n, l, col_max, col_sumsq, b_norm):
    """(s_safe, gap+, rho+) from the certificate's record [||r||^2, <r, b>, sum ||x_i||, gmax, ...]:
    the issue's three errors, term by term, in float64.
      1. s_safe = min(1, mu / (gmax + gamma_m cmax ||r||));
      2. delta_r = gamma_n ||A||_F sum ||x_i|| + eps (||r|| + 2 ||b||); the primal value is off by at
         most ||r|| delta_r + delta_r^2 / 2, plus the bars of the fp64 sums ||r||^2, <r, b> (m l + 2
         terms each) and sum ||x_i|| (a row norm in A's dtype, then n + 2 terms in double);
      3. rho+ = sqrt(2 gap+) + s gamma_m ||r|| + s gamma_l (1 + gamma_m) ||r||, times
         1 + gamma64_{m+2} for the stored column norms."""
    rr, rb, sx, gmax = (float(v) for v in rec[:4])
    rn = np.sqrt(rr)
    gm, gn = gamma(m + 2, eps), gamma(n + 2, eps)
    den = gmax + gm * col_max * rn
    s = mu / den if den > mu else (1.0 if den <= mu else den)
    dr = gn * np.sqrt(col_sumsq) * sx + eps * (rn + 2.0 * b_norm)
    g_ml = gamma(float(m) * float(l) + 2.0, EPS64)
    bar_rr = g_ml * rr
    bar_rb = g_ml * rn * b_norm
    bar_sx = (gamma(l + 2, eps) + gamma(n + 2, EPS64)) * sx
    gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * sx
    bars = rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx
    gap_p = (gap if gap > 0.0 else (0.0 if gap <= 0.0 else gap)) + bars
    gl = gamma(l + 2, eps)
    rho = np.sqrt(2.0 * gap_p) + s * gm * rn + s * gl * (1.0 + gm) * rn
    rho *= 1.0 + gamma(m + 2, EPS64)
    return float(s), float(gap_p), float(rho)


def primal_bar(rec, mu, eps, m, n, l, col_sumsq, b_norm):
    """How far the primal value composed from the record, 1/2 ||r^||^2 + mu sum ||x_i||, can be from
    P(x): the guard's item 2 with its sums' bars (the dual's terms left out)."""
    rr, _, sx = (float(v) for v in rec[:3])
    rn = np.sqrt(rr)
    dr = gamma(n + 2, eps) * np.sqrt(col_sumsq) * sx + eps * (rn + 2.0 * b_norm)
    bar_rr = gamma(float(m) * float(l) + 2.0, EPS64) * rr
    bar_sx = (gamma(l + 2, eps) + gamma(n + 2, EPS64)) * sx
    return float(rn * dr + 0.5 * dr * dr + 0.5 * bar_rr + mu * bar_sx)


def record(cert):
    """The eight-value record glx_certificate would return, from certificate_ref.certificate's dict."""
    return [float(cert["rr"]), float(cert["rb"]), float(cert["sum_xnorm"]), float(cert["gmax"]),
            float(cert["kkt_max"]), float(cert["kkt_sq"]), float(cert["nonzero_rows"]), 0.0]


def prox(w, tmu):
    nrm = np.sqrt(np.sum(w * w, axis=1))
    scale = np.where(nrm > tmu, 1.0 - tmu / np.where(nrm > 0, nrm, 1.0), 0.0)
    return w * scale[:, None]


def fista_screen(A, b, mu, x0=None, tol=1e-8, maxit=200000, screen=True, check_every=10, restart=True):
    """FISTA with the exact prox, the step 1 / lambda_max(A^T A) and guarded gap-safe screening, in
    float64 on the columns still kept. Returns (x (n x l), info) with info = {"iterations", "kept"
    (bool mask of the rows not screened), "rel_gap", "kept_history"}. restart: the gradient scheme of
    adaptive restart (the momentum is dropped when it points uphill), which the GPU loop does not
    use; it only makes the reference converge linearly."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    m, n = A.shape
    l = b.shape[1]
    t = 1.0 / float(np.linalg.eigvalsh(A.T @ A)[-1])
    cn_all = np.asarray(col_norms(A), dtype=np.float64)
    cmax, csq, bn = float(cn_all.max()), float(np.sum(cn_all ** 2)), float(np.linalg.norm(b))
    idx = np.arange(n)
    Ac = A
    x = np.zeros((n, l)) if x0 is None else np.array(x0, dtype=np.float64)
    y = x.copy()
    k = 1
    hist = []
    rel = np.inf
    it = 0
    while True:
        if it % check_every == 0 or it >= maxit:
            c = cref.certificate(x, Ac, b, mu)
            rel = float(c["rel_gap"])
            if rel <= tol or it >= maxit:
                break
            if screen:
                s, _, rho = guard(record(c), mu, EPS64, m, Ac.shape[1], l, cmax, csq, bn)
                keep = keep_mask(c["row_norms"], cn_all[idx], s, rho, mu * (1.0 - 4.0 * EPS64))
                if not keep.all():
                    idx, Ac, x = idx[keep], Ac[:, keep], x[keep]
                    y, k = x.copy(), 1
                    hist.append(int(keep.sum()))
                    if idx.size == 0:
                        break
        theta, theta_next = 2.0 / (k + 1), 2.0 / (k + 2)
        g = Ac.T @ (Ac @ y - b)
        xc = prox(y - t * g, t * mu)
        if restart and float(np.sum((y - xc) * (xc - x))) > 0.0:
            y, k = xc.copy(), 1
        else:
            v = x + (xc - x) / theta
            y = (1.0 - theta_next) * xc + theta_next * v
            k += 1
        x = xc
        it += 1
    full = np.zeros((n, l))
    full[idx] = x
    kept = np.zeros(n, dtype=bool)
    kept[idx] = True
    return full, {"iterations": it, "kept": kept, "rel_gap": rel, "kept_history": hist}


@functools.lru_cache(maxsize=None)
def reference_solution(seed, m, n, l, ratio, f32=False):
    """The instance of glx.driver.gen_data(seed, m, n, l) at mu = ratio * mu_max and its reference
    solution: float64 FISTA with restarts and screening down to the float64 gap's floor, then the
    certificate of the result in longdouble, which must show rel_gap <= 1e-12. Returns a dict: A, b,
    mu (float64), x (float64), theta (longdouble A x - b), gtheta (longdouble ||a_i^T theta||, n),
    primal, dual, gap (longdouble). f32: A and b rounded to float32 first. Computed once per case and shared (do not modify)."""
    A, b, _, _ = cref.instance(seed, m, n, l)
    if f32:   # the instance a float32 solve sees, held exactly in float64
        A, b = A.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    mu = float(ratio) * float(cref.mu_max(A, b))
    x, info = fista_screen(A, b, mu, tol=2e-14, maxit=400000)
    c = cref.certificate(x.astype(LD), A.astype(LD), b.astype(LD), LD(mu))
    assert float(c["rel_gap"]) <= 1e-12, ("the reference did not reach 1e-12", float(c["rel_gap"]), info)
    for a in (A, b, x):
        a.setflags(write=False)
    return {"A": A, "b": b, "mu": mu, "x": x, "theta": c["r"], "gtheta": c["row_norms"],
            "primal": c["primal"], "dual": c["dual"], "gap": c["gap"], "iterations": info["iterations"]}
