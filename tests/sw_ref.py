"""Sample weights and cross-validation (DESIGN.md "Sample weights and cross-validation") in NumPy:
the test reference.

    P_w(x) = 1/2 sum_j w_j ||(A x - b)_j||^2 + mu Omega(x),   w_j >= 0, one per row j of A,

is the unweighted problem on (A~, b~) = (sqrt(w) o A, sqrt(w) o b), so every weighted quantity here is
an existing reference (certificate_ref, screen_ref, group_ref) applied to that pair: the library
never forms it, the reference always does. Also holds the mirrors of the two weighted rounding
guards (term by term, as screen_ref.guard and group_ref.guard mirror the unweighted ones), the fold
helpers and the cross-validation aggregate, written independently of glx.cv. Imports nothing from
glx except, through certificate_ref, the instance generator.
"""
import functools

import numpy as np

import certificate_ref as cref
import group_ref as gr
import screen_ref as sr

LD = np.longdouble
EPS64 = sr.EPS64
EPS32 = sr.EPS32
gamma = sr.gamma


def reduce(A, b, w, wide=np.float64):
    """(sqrt(w) o A, sqrt(w) o b) in `wide`."""
    s = np.sqrt(np.asarray(w).astype(wide))[:, None]
    return s * np.asarray(A).astype(wide), s * np.asarray(b).astype(wide)


def draw_weights(seed, m):
    """The issue's general weights: uniform in [0, 3] with a quarter of them exactly zero."""
    g = np.random.default_rng(seed)
    w = g.uniform(0.0, 3.0, m)
    w[g.choice(m, size=m // 4, replace=False)] = 0.0
    return w


def certificate(x, A, b, mu, w, ptr=None, gw=None, wide=LD):
    """The weighted certificate in `wide`: certificate_ref's (rows) or group_ref's (ptr, gw) on the
    reduced pair. "rr" = sum w r^2 and "rb" = sum w r b; "r" is sqrt(w) o (A x - b)."""
    At, bt = reduce(A, b, w, wide)
    if ptr is None:
        return cref.certificate(np.asarray(x).astype(wide), At, bt, wide(mu))
    return gr.certificate(np.asarray(x).astype(wide), At, bt, wide(mu), ptr, gw)


def mu_max(A, b, w, ptr=None, gw=None, wide=LD):
    At, bt = reduce(A, b, w, wide)
    if ptr is None:
        return cref.mu_max(At, bt)
    return np.max(gr.group_norms(At.T @ bt, ptr) / np.asarray(gw).astype(wide))


def col_norms(A, w, wide=LD):
    """sqrt(sum_j w_j A_ji^2) in `wide`."""
    a = np.asarray(A).astype(wide)
    return np.sqrt(np.sum(np.asarray(w).astype(wide)[:, None] * a * a, axis=0))


def primal(x, A, b, mu, w, ptr=None, gw=None, wide=LD):
    """P_w(x) in `wide`, formed on the ORIGINAL A and b (no square roots)."""
    r = np.asarray(A).astype(wide) @ np.asarray(x).astype(wide) - np.asarray(b).astype(wide)
    loss = np.sum(np.asarray(w).astype(wide)[:, None] * r * r) / 2
    xl = np.asarray(x).astype(wide)
    if ptr is None:
        pen = np.sum(np.sqrt(np.sum(xl * xl, axis=1)))
    else:
        pen = np.sum(np.asarray(gw).astype(wide) * gr.group_norms(xl, ptr))
    return loss + wide(mu) * pen


def holdout_loss(x, A, b, v, wide=LD):
    """1/2 sum_j v_j ||(A x - b)_j||^2 / sum_j v_j in `wide`."""
    r = np.asarray(A).astype(wide) @ np.asarray(x).astype(wide) - np.asarray(b).astype(wide)
    vv = np.asarray(v).astype(wide)
    return np.sum(vv[:, None] * r * r) / 2 / np.sum(vv)


# ------------------------------------------------------------------------------------------ guards
def guard(rec, mu, eps, m, n, l, col_max, col_sumsq, b_norm):
    """(s_safe, gap+, rho+) of glx_screen_guard_sw in float64, term by term: screen_ref.guard with the
    weighted record (rec[0] = sum w r^2, rec[1] = sum w r b), the weighted column figures and
    b_norm = ||b~||, and k = 3 in place of 2 where the weights add a rounding:
      1. the A^T pass runs on fl(w r^): gamma_{m+3}(eps) in place of gamma_{m+2};
      2. (w r^) r^ and (w r^) b in the fp64 sums: gamma64_{ml+3}; ||b~|| is itself such a sum's root
         and is raised by 1 + gamma64_{ml+3};
      3. (w a) a in the column norms: the stored norms are low by at most gamma64_{m+3}."""
    rr, rb, sx, gmax = (float(v) for v in rec[:4])
    rn = np.sqrt(rr)
    gm, gn = gamma(m + 3, eps), gamma(n + 2, eps)
    g_ml = gamma(float(m) * float(l) + 3.0, EPS64)
    bn = b_norm * (1.0 + g_ml)
    den = gmax + gm * col_max * rn
    s = mu / den if den > mu else (1.0 if den <= mu else den)
    dr = gn * np.sqrt(col_sumsq) * sx + eps * (rn + 2.0 * bn)
    bar_rr = g_ml * rr
    bar_rb = g_ml * rn * bn
    bar_sx = (gamma(l + 2, eps) + gamma(n + 2, EPS64)) * sx
    gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * sx
    bars = rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx
    gap_p = (gap if gap > 0.0 else (0.0 if gap <= 0.0 else gap)) + bars
    gl = gamma(l + 2, eps)
    rho = np.sqrt(2.0 * gap_p) + s * gm * rn + s * gl * (1.0 + gm) * rn
    rho *= 1.0 + gamma(m + 3, EPS64)
    return float(s), float(gap_p), float(rho)


def group_guard(rec, mu, eps, m, n, l, max_run, w_min, gcol_max, col_sumsq, b_norm):
    """glx_group_screen_guard_sw in float64: group_ref.guard with the same three substitutions."""
    rr, rb, sxw, gmax = (float(v) for v in rec[:4])
    rn = np.sqrt(rr)
    gm, gn = gamma(m + 3, eps), gamma(n + 2, eps)
    gK = gamma(float(max_run) * float(l) + 3.0, eps)
    g_ml = gamma(float(m) * float(l) + 3.0, EPS64)
    bn = b_norm * (1.0 + g_ml)
    up = (1.0 + gamma(m + 3, EPS64)) * (1.0 + gamma(max_run + 3, EPS64))
    den = gmax * (1.0 + gK) + gm * gcol_max * up * rn
    s = mu / den if den > mu else (1.0 if den <= mu else den)
    dr = gn * np.sqrt(col_sumsq) * (sxw / w_min) + eps * (rn + 2.0 * bn)
    bar_rr = g_ml * rr
    bar_rb = g_ml * rn * bn
    bar_sx = (gK + gamma(n + 2, EPS64)) * sxw
    gap = 0.5 * (1.0 + s * s) * rr + s * rb + mu * sxw
    bars = rn * dr + 0.5 * dr * dr + 0.5 * (1.0 + s * s) * bar_rr + s * bar_rb + mu * bar_sx
    gap_p = (gap if gap > 0.0 else (0.0 if gap <= 0.0 else gap)) + bars
    rho = np.sqrt(2.0 * gap_p) + s * gm * rn + s * gK * (1.0 + gm) * rn
    rho *= up
    return float(s), float(gap_p), float(rho)


def primal_bar(rec, mu, eps, m, n, l, col_sumsq, b_norm):
    """screen_ref.primal_bar with the weighted figures: how far 1/2 rec[0] + mu rec[2] can be from
    P_w(x) (the guard's item 2 and its sums' bars, gamma64_{ml+3} for the weighted sum)."""
    rr, _, sx = (float(v) for v in rec[:3])
    rn = np.sqrt(rr)
    g_ml = gamma(float(m) * float(l) + 3.0, EPS64)
    dr = gamma(n + 2, eps) * np.sqrt(col_sumsq) * sx + eps * (rn + 2.0 * b_norm * (1.0 + g_ml))
    bar_sx = (gamma(l + 2, eps) + gamma(n + 2, EPS64)) * sx
    return float(rn * dr + 0.5 * dr * dr + 0.5 * g_ml * rr + mu * bar_sx)


def group_primal_bar(rec, mu, eps, m, n, l, max_run, w_min, col_sumsq, b_norm):
    rr, _, sxw = (float(v) for v in rec[:3])
    rn = np.sqrt(rr)
    g_ml = gamma(float(m) * float(l) + 3.0, EPS64)
    dr = gamma(n + 2, eps) * np.sqrt(col_sumsq) * (sxw / w_min) + eps * (rn + 2.0 * b_norm * (1.0 + g_ml))
    bar_sx = (gamma(float(max_run) * float(l) + 3.0, eps) + gamma(n + 2, EPS64)) * sxw
    return float(rn * dr + 0.5 * dr * dr + 0.5 * g_ml * rr + mu * bar_sx)


# ------------------------------------------------------------------------------------------ solutions
SEED = 1            # the gen_data seed of the screen tests
WSEED = 7           # the seed of the general weights


def weights_of(kind, m):
    """The weight vectors of the solve tests, float64: "general" (draw_weights), "mask" (rows
    j mod 4 != 0), "int" (1, 2, 3 cycling by a seeded draw), "ones"."""
    if kind == "general":
        return draw_weights(WSEED, m)
    if kind == "mask":
        return (np.arange(m) % 4 != 0).astype(np.float64)
    if kind == "int":
        return np.random.default_rng(WSEED + 1).integers(1, 4, m).astype(np.float64)
    if kind == "ones":
        return np.ones(m)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def reference_solution(m, n, l, ratio, kind="general", f32=False):
    """The instance of glx.driver.gen_data(SEED, m, n, l) with the weights `kind` at mu = ratio times
    the weighted mu_max, and its reference solution: screen_ref.reference_solution's recipe on the
    reduced pair (float64 FISTA with restarts and guarded screening to the gap's floor, then the
    certificate in longdouble, which must show rel_gap <= 1e-12). Returns a dict: A, b, w (float64, the
    originals), mu, x, gtheta (longdouble ||a~_i^T theta~||), primal, dual, gap (longdouble).
    Shared: do not modify."""
    A, b, _, _ = cref.instance(SEED, m, n, l)
    w = weights_of(kind, m)
    if f32:
        A, b = A.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
        w = w.astype(np.float32).astype(np.float64)
    At, bt = reduce(A, b, w)
    mu = float(ratio) * float(cref.mu_max(At, bt))
    x, info = sr.fista_screen(At, bt, mu, tol=2e-14, maxit=400000)
    c = certificate(x, A, b, mu, w)
    assert float(c["rel_gap"]) <= 1e-12, ("the reference did not reach 1e-12", float(c["rel_gap"]), info)
    for a in (A, b, w, x):
        a.setflags(write=False)
    return {"A": A, "b": b, "w": w, "mu": mu, "x": x, "gtheta": c["row_norms"], "primal": c["primal"],
            "dual": c["dual"], "gap": c["gap"], "iterations": info["iterations"]}


GROUP_SIZES = (1, 2, 3, 5, 8)


@functools.lru_cache(maxsize=None)
def group_reference_solution(m, n, l, ratio):
    """The grouped case: gen_data's instance, general weights, groups of sizes drawn from
    [1, 2, 3, 5, 8] (seeded) with weights sqrt(size); group_ref.fista_screen on the reduced pair."""
    A, b, _, _ = cref.instance(SEED, m, n, l)
    w = weights_of("general", m)
    ptr = gr.draw_groups(np.random.default_rng(WSEED + 2), n, GROUP_SIZES)
    gw = np.sqrt(np.diff(ptr).astype(np.float64))
    At, bt = reduce(A, b, w)
    mu = float(ratio) * float(gr.mu_max(At, bt, ptr, gw))
    x, info = gr.fista_screen(At, bt, mu, ptr, gw, tol=2e-14)
    c = certificate(x, A, b, mu, w, ptr, gw)
    assert float(c["rel_gap"]) <= 1e-12, ("the reference did not reach 1e-12", float(c["rel_gap"]), info)
    for a in (A, b, w, x, ptr, gw):
        a.setflags(write=False)
    return {"A": A, "b": b, "w": w, "ptr": ptr, "gw": gw, "mu": mu, "x": x, "gtheta": c["group_norms"],
            "primal": c["primal"], "dual": c["dual"], "gap": c["gap"]}


# ------------------------------------------------------------------------------------------ folds and CV
def fold_vectors(labels, k, w=None):
    """(training, hold-out) weights of fold k."""
    lab = np.asarray(labels)
    base = np.ones(lab.size) if w is None else np.asarray(w, dtype=np.float64)
    return base * (lab != k), base * (lab == k)


def cv_aggregate(fold_loss):
    """(mean, se, best, one_se) of a K x n_mus table, written out by hand."""
    fl = np.asarray(fold_loss, dtype=np.float64)
    K, nm = fl.shape
    mean = np.array([sum(fl[k, i] for k in range(K)) / K for i in range(nm)])
    se = np.array([np.sqrt(sum((fl[k, i] - mean[i]) ** 2 for k in range(K)) / (K - 1) / K) for i in range(nm)])
    best = min(range(nm), key=lambda i: (mean[i], i))
    one_se = next(i for i in range(nm) if mean[i] <= mean[best] + se[best])
    return mean, se, best, one_se


def cv_instance():
    """The issue's cross-validation instance: default_rng(3), A 120 x 256 standard normal, 12 active
    rows of u (l = 4), b = A u + 2 noise."""
    g = np.random.default_rng(3)
    A = g.standard_normal((120, 256))
    u = np.zeros((256, 4))
    u[g.choice(256, 12, replace=False)] = g.standard_normal((12, 4))
    b = A @ u + 2.0 * g.standard_normal((120, 4))
    return A, b


def cv_reference(A, b, K=5, n_mus=10, mu_min_ratio=1e-2, tol=1e-8):
    """The reference curve: for every fold j mod K, the warm-started path of screen_ref.fista_screen on
    the reduced training pair over the full data's geometric grid, and the hold-out loss of each
    solution. Returns (mus, fold_loss K x n_mus)."""
    m = A.shape[0]
    top = float(cref.mu_max(A, b))
    q = mu_min_ratio ** (1.0 / (n_mus - 1))
    mus = [top * q ** i for i in range(n_mus)]
    labels = np.arange(m) % K
    fl = np.zeros((K, n_mus))
    for k in range(K):
        tr, ho = fold_vectors(labels, k)
        At, bt = reduce(A, b, tr)
        x = None
        for i, mu in enumerate(mus):
            x, _ = sr.fista_screen(At, bt, mu, x0=x, tol=tol)
            fl[k, i] = float(holdout_loss(x, A, b, ho, np.float64))
    return mus, fl
