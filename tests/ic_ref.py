"""An unpenalised intercept (DESIGN.md "Intercept") in NumPy: the test reference.

    P(x, c) = 1/2 sum_j w_j ||(A x + 1 c^T - b)_j||^2 + mu Omega(x),   c in R^l unpenalised.

For fixed x the minimiser is c(x) = -r-bar, the weighted column mean of r = A x - b, so min_c P(x, c) is
the intercept-free problem on the pair (P~ A~, P~ b~) with A~ = sqrt(w) o A, b~ = sqrt(w) o b,
1~ = sqrt(w) and P~ = I - 1~ 1~^T / sigma. Every quantity here is an existing reference
(certificate_ref, screen_ref, group_ref) applied to that pair, which this module forms explicitly and
the library never does. Also holds the mirrors of the two guards (term by term, as sw_ref mirrors the
weighted ones), the offset instance of the tests and the cross-validation reference with an
intercept per fold. Imports nothing from glx except, through certificate_ref, the instance generator.
"""
import functools

import numpy as np

import certificate_ref as cref
import group_ref as gr
import screen_ref as sr
import sw_ref as sw

LD = np.longdouble
EPS64 = sr.EPS64
EPS32 = sr.EPS32
gamma = sr.gamma
SEED = sw.SEED


def offset_instance(m, n, l):
    """The offset instance: gen_data(1, m, n, l) with default_rng(11) offsets, one per column of A added
    to every row, then 3 times one per column of b."""
    A, b, _, _ = cref.instance(SEED, m, n, l)
    g = np.random.default_rng(11)
    A = A + g.standard_normal(n)[None, :]
    b = b + 3.0 * g.standard_normal(l)[None, :]
    return np.ascontiguousarray(A), np.ascontiguousarray(b)


def centre(A, b, w, wide=np.float64):
    """(P~ A~, P~ b~) in `wide`."""
    At, bt = sw.reduce(A, b, w, wide)
    one = np.sqrt(np.asarray(w).astype(wide))[:, None]
    sigma = np.sum(np.asarray(w).astype(wide))
    return At - one * ((one.T @ At) / sigma), bt - one * ((one.T @ bt) / sigma)


def intercept_of(x, A, b, w, wide=LD):
    """c(x) = -(weighted column mean of A x - b), l values in `wide`."""
    r = np.asarray(A).astype(wide) @ np.asarray(x).astype(wide) - np.asarray(b).astype(wide)
    ww = np.asarray(w).astype(wide)
    return -(ww @ r) / np.sum(ww)


def certificate(x, A, b, mu, w, ptr=None, gw=None, wide=LD):
    """The certificate of min_c P(x, c) in `wide`: certificate_ref's (rows) or group_ref's (ptr, gw) on the
    centred pair, plus "intercept" = c(x). "r" is sqrt(w) o r_c."""
    Ac, bc = centre(A, b, w, wide)
    if ptr is None:
        c = cref.certificate(np.asarray(x).astype(wide), Ac, bc, wide(mu))
    else:
        c = gr.certificate(np.asarray(x).astype(wide), Ac, bc, wide(mu), ptr, gw)
    c["intercept"] = intercept_of(x, A, b, w, wide)
    return c


def mu_max(A, b, w, ptr=None, gw=None, wide=LD):
    Ac, bc = centre(A, b, w, wide)
    if ptr is None:
        return cref.mu_max(Ac, bc)
    return np.max(gr.group_norms(Ac.T @ bc, ptr) / np.asarray(gw).astype(wide))


def col_means(A, w, wide=LD):
    ww = np.asarray(w).astype(wide)
    return (ww @ np.asarray(A).astype(wide)) / np.sum(ww)


def col_norms(A, w, wide=LD):
    """The centred weighted norms sqrt(sum_j w_j (A_ji - a-bar_i)^2) in `wide`."""
    a = np.asarray(A).astype(wide)
    d = a - col_means(A, w, wide)[None, :]
    return np.sqrt(np.sum(np.asarray(w).astype(wide)[:, None] * d * d, axis=0))


def col_stats(A, w):
    """glx_col_norms_ic's four statistics in float64 from longdouble figures: [max centred norm, sum of
    their squares, max |column mean|, sum of the squared means]."""
    cn, am = col_norms(A, w), col_means(A, w)
    return [float(cn.max()), float(np.sum(cn * cn)), float(np.max(np.abs(am))), float(np.sum(am * am))]


def primal(x, c, A, b, mu, w, ptr=None, gw=None, wide=LD):
    """P(x, c) in `wide`, formed on the ORIGINAL A and b with the intercept c given explicitly."""
    r = (np.asarray(A).astype(wide) @ np.asarray(x).astype(wide) + np.asarray(c).astype(wide)[None, :]
         - np.asarray(b).astype(wide))
    loss = np.sum(np.asarray(w).astype(wide)[:, None] * r * r) / 2
    xl = np.asarray(x).astype(wide)
    if ptr is None:
        pen = np.sum(np.sqrt(np.sum(xl * xl, axis=1)))
    else:
        pen = np.sum(np.asarray(gw).astype(wide) * gr.group_norms(xl, ptr))
    return loss + wide(mu) * pen


def holdout_loss(x, c, A, b, v, wide=LD):
    """1/2 sum_j v_j ||(A x + c - b)_j||^2 / sum_j v_j in `wide`."""
    r = (np.asarray(A).astype(wide) @ np.asarray(x).astype(wide) + np.asarray(c).astype(wide)[None, :]
         - np.asarray(b).astype(wide))
    vv = np.asarray(v).astype(wide)
    return np.sum(vv[:, None] * r * r) / 2 / np.sum(vv)


# ------------------------------------------------------------------------------------------ guards
def guard(rec, mu, eps, m, n, l, cstats, b_norm, sigma, mean_sq):
    """(s_safe, gap+, rho+, slack) of glx_screen_guard_ic in float64, term by term: sw_ref.guard on the
    centred record (rec[0] = sum w r_c^2, rec[1] = sum w r_c b) with
      1. the uncentred figures by Pythagoras, raised by py for their own roundings: cu^2 = cmax^2 up^2 +
         sigma amax^2, csq_u = csq + sigma asq, rhn^2 = rec[0] + sigma mean_sq (and r_c's rounding);
      2. eps_c = gamma_2(eps) ||r~_c|| + gamma64_{m+3} ||r~^||, the departure from 1~^T theta = 0: in the
         feasibility denominator (times amax sqrt(sigma)), in the dual value (s eps_c ||b~|| +
         1/2 s^2 eps_c^2) and in the radius (s eps_c);
      3. one more rounding of the residual in dr (eps ||r~_c||), whose product part sees ||r~^||;
      4. the centred norms low by gamma64_{m+5}: (w d) d with d = a - a-bar rounded in double;
      5. the slack: the rounding terms that scale with the uncentred norm, taken off mu."""
    rr, rb, sx, gmax = (float(v) for v in rec[:4])
    cmax, csq, amax, asq = (float(v) for v in cstats)
    rn = np.sqrt(rr)
    gm, gn = gamma(m + 3, eps), gamma(n + 2, eps)
    g_ml = gamma(float(m) * float(l) + 3.0, EPS64)
    bn = b_norm * (1.0 + g_ml)
    up = 1.0 + gamma(m + 5, EPS64)
    py = 1.0 + 3.0 * gamma(float(m) + float(n) + 8.0, EPS64)
    cu = np.sqrt((cmax * cmax * up * up + sigma * amax * amax) * py)
    csq_u = (csq + sigma * asq) * py
    rhn = np.sqrt((rr + sigma * mean_sq) * py * (1.0 + 4.0 * eps))
    eps_c = gamma(2, eps) * rn + gamma(m + 3, EPS64) * rhn
    dep = amax * np.sqrt(sigma) * eps_c * (1.0 + 4.0 * EPS64)
    den = gmax + gm * cu * rn + dep
    s = mu / den if den > mu else (1.0 if den <= mu else den)
    dr = gn * np.sqrt(csq_u) * sx + eps * (rhn + 2.0 * bn) + eps * rn
    bar_rr = g_ml * rr
    bar_rb = g_ml * rn * bn
    bar_sx = (gamma(l + 2, eps) + gamma(n + 2, EPS64)) * sx
    gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * sx
    bars = (rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx
            + s * eps_c * bn + 0.5 * s * s * eps_c * eps_c)
    gap_p = (gap if gap > 0.0 else (0.0 if gap <= 0.0 else gap)) + bars
    gl = gamma(l + 2, eps)
    rho = (np.sqrt(2.0 * gap_p) + s * eps_c) * up
    slack = s * (gm * cu * rn + gl * (1.0 + gm) * cu * rn + dep) * (1.0 + 8.0 * EPS64)
    return float(s), float(gap_p), float(rho), float(slack)


def group_guard(rec, mu, eps, m, n, l, max_run, w_min, gcol_max, cstats, b_norm, sigma, mean_sq):
    """glx_group_screen_guard_ic in float64: sw_ref.group_guard with the same substitutions; a group's mean
    part is at most ga = sqrt(max_run sigma) amax / w_min."""
    rr, rb, sxw, gmax = (float(v) for v in rec[:4])
    _, csq, amax, asq = (float(v) for v in cstats)
    rn = np.sqrt(rr)
    gm, gn = gamma(m + 3, eps), gamma(n + 2, eps)
    gK = gamma(float(max_run) * float(l) + 3.0, eps)
    g_ml = gamma(float(m) * float(l) + 3.0, EPS64)
    bn = b_norm * (1.0 + g_ml)
    up = (1.0 + gamma(m + 5, EPS64)) * (1.0 + gamma(max_run + 3, EPS64))
    py = 1.0 + 3.0 * gamma(float(m) + float(n) + 8.0, EPS64)
    ga = np.sqrt(float(max_run) * sigma) * amax / w_min
    gcu = np.sqrt((gcol_max * gcol_max * up * up + ga * ga) * py)
    csq_u = (csq + sigma * asq) * py
    rhn = np.sqrt((rr + sigma * mean_sq) * py * (1.0 + 4.0 * eps))
    eps_c = gamma(2, eps) * rn + gamma(m + 3, EPS64) * rhn
    dep = ga * eps_c * (1.0 + 4.0 * EPS64)
    den = gmax * (1.0 + gK) + gm * gcu * rn + dep
    s = mu / den if den > mu else (1.0 if den <= mu else den)
    dr = gn * np.sqrt(csq_u) * (sxw / w_min) + eps * (rhn + 2.0 * bn) + eps * rn
    bar_rr = g_ml * rr
    bar_rb = g_ml * rn * bn
    bar_sx = (gK + gamma(n + 2, EPS64)) * sxw
    gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * sxw
    bars = (rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx
            + s * eps_c * bn + 0.5 * s * s * eps_c * eps_c)
    gap_p = (gap if gap > 0.0 else (0.0 if gap <= 0.0 else gap)) + bars
    rho = (np.sqrt(2.0 * gap_p) + s * eps_c) * up
    slack = s * (gm * gcu * rn + gK * (1.0 + gm) * gcu * rn + dep) * (1.0 + 8.0 * EPS64)
    return float(s), float(gap_p), float(rho), float(slack)


def figures(A, b, w):
    """(cstats, ||b~||, sigma) of the guard for this instance, float64 from longdouble."""
    wl = np.asarray(w).astype(LD)
    bn = float(np.sqrt(np.sum(wl[:, None] * np.asarray(b).astype(LD) ** 2)))
    return col_stats(A, w), bn, float(np.sum(wl))


# ------------------------------------------------------------------------------------------ solutions
@functools.lru_cache(maxsize=None)
def reference_solution(m, n, l, ratio, kind="general", f32=False):
    """The offset instance with the weights `kind` (sw_ref.weights_of) at mu = ratio times the intercept
    problem's mu_max, and its reference solution: sw_ref.reference_solution's recipe on the centred pair
    (float64 FISTA with restarts and guarded screening to the gap's floor, then the certificate in
    longdouble, which must show rel_gap <= 1e-12). Returns a dict: A, b, w (float64, the originals), mu,
    x, c (the intercept, longdouble), gtheta (longdouble ||(P~ a~_i)^T theta||), primal, dual, gap.
    Shared: do not modify."""
    A, b = offset_instance(m, n, l)
    w = sw.weights_of(kind, m)
    if f32:
        A, b = A.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
        w = w.astype(np.float32).astype(np.float64)
    Ac, bc = centre(A, b, w)
    mu = float(ratio) * float(cref.mu_max(Ac, bc))
    x, info = sr.fista_screen(Ac, bc, mu, tol=2e-14, maxit=400000)
    c = certificate(x, A, b, mu, w)
    assert float(c["rel_gap"]) <= 1e-12, ("the reference did not reach 1e-12", float(c["rel_gap"]), info)
    for a in (A, b, w, x):
        a.setflags(write=False)
    return {"A": A, "b": b, "w": w, "mu": mu, "x": x, "c": c["intercept"], "gtheta": c["row_norms"],
            "primal": c["primal"], "dual": c["dual"], "gap": c["gap"], "iterations": info["iterations"]}


@functools.lru_cache(maxsize=None)
def group_reference_solution(m, n, l, ratio):
    """The grouped case: the offset instance, general weights, sw_ref's groups and group weights;
    group_ref.fista_screen on the centred pair."""
    A, b = offset_instance(m, n, l)
    w = sw.weights_of("general", m)
    ptr = gr.draw_groups(np.random.default_rng(sw.WSEED + 2), n, sw.GROUP_SIZES)
    gw = np.sqrt(np.diff(ptr).astype(np.float64))
    Ac, bc = centre(A, b, w)
    mu = float(ratio) * float(gr.mu_max(Ac, bc, ptr, gw))
    x, info = gr.fista_screen(Ac, bc, mu, ptr, gw, tol=2e-14)
    c = certificate(x, A, b, mu, w, ptr, gw)
    assert float(c["rel_gap"]) <= 1e-12, ("the reference did not reach 1e-12", float(c["rel_gap"]), info)
    for a in (A, b, w, x, ptr, gw):
        a.setflags(write=False)
    return {"A": A, "b": b, "w": w, "ptr": ptr, "gw": gw, "mu": mu, "x": x, "c": c["intercept"],
            "gtheta": c["group_norms"], "primal": c["primal"], "dual": c["dual"], "gap": c["gap"]}


# ------------------------------------------------------------------------------------------ CV
def cv_instance():
    """sw_ref.cv_instance() with the offset instance's offsets (default_rng(11)): one per column of A, then
    3 times one per column of b."""
    A, b = sw.cv_instance()
    g = np.random.default_rng(11)
    A = A + g.standard_normal(A.shape[1])[None, :]
    b = b + 3.0 * g.standard_normal(b.shape[1])[None, :]
    return np.ascontiguousarray(A), np.ascontiguousarray(b)


def cv_reference(A, b, K=5, n_mus=10, mu_min_ratio=1e-2, tol=1e-8):
    """The reference curve with an intercept per fold: the grid from the full data's intercept mu_max; for
    every fold j mod K the warm-started path of screen_ref.fista_screen on the centred training pair, and
    the hold-out loss of each solution with its training intercept. Returns (mus, fold_loss K x n_mus)."""
    m = A.shape[0]
    top = float(mu_max(A, b, np.ones(m), wide=np.float64))
    q = mu_min_ratio ** (1.0 / (n_mus - 1))
    mus = [top * q ** i for i in range(n_mus)]
    labels = np.arange(m) % K
    fl = np.zeros((K, n_mus))
    for k in range(K):
        tr, ho = sw.fold_vectors(labels, k)
        Ac, bc = centre(A, b, tr)
        x = None
        for i, mu in enumerate(mus):
            x, _ = sr.fista_screen(Ac, bc, mu, x0=x, tol=tol)
            c = intercept_of(x, A, b, tr, np.float64)
            fl[k, i] = float(holdout_loss(x, c, A, b, ho, np.float64))
    return mus, fl
