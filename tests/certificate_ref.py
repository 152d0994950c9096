"""The optimality certificate (DESIGN.md "Certificate") in NumPy: the test reference.

For P(x) = 1/2 ||A x - b||_F^2 + mu sum_i ||x_i||_2 and its dual D(theta) = -1/2 ||theta||_F^2 -
<theta, b> over ||(A^T theta)_i||_2 <= mu: r = A x - b, g = A^T r, gmax = max_i ||g_i||,
s = 1 where gmax <= mu and mu / gmax elsewhere, gap = P(x) - D(s r); the KKT violation of row i is
||g_i + mu x_i / ||x_i|| || where x_i != 0 and max(||g_i|| - mu, 0) where x_i = 0.

Imports nothing from glx except the instance generator ``glx.driver.gen_data``. Every function
computes in the dtype of its inputs (``np.longdouble`` for a wider-than-double reference).
"""
import numpy as np


def instance(seed, m, n, l, mu=1e-2):
    """(A, b, x0, mu) of glx.driver.gen_data."""
    from glx.driver import gen_data
    _, _, _, mu, A, b, _u, x0, *_ = gen_data(seed, m, n, l, mu)
    return A, b, x0, mu


def row_terms(x, g, mu):
    """The per-row quantities on a given g: {"xnorm", "gnorm", "kkt"} (length n) and the five sums
    [sum ||x_i||, max ||g_i||, max kkt_i, sum kkt_i^2, #{x_i != 0}]. A row is zero when its norm is."""
    dt = np.result_type(x.dtype, g.dtype)
    x = x.astype(dt)
    g = g.astype(dt)
    mu = dt.type(mu)
    xn = np.sqrt(np.sum(x * x, axis=1))
    gn = np.sqrt(np.sum(g * g, axis=1))
    nz = xn != 0
    safe = np.where(nz, xn, dt.type(1))
    k_nz = np.sqrt(np.sum((g + mu * x / safe[:, None]) ** 2, axis=1))
    k_z = np.maximum(gn - mu, dt.type(0))
    kkt = np.where(nz, k_nz, k_z)
    sums = [np.sum(xn), np.max(gn), np.max(kkt), np.sum(kkt * kkt), dt.type(np.count_nonzero(nz))]
    return {"xnorm": xn, "gnorm": gn, "kkt": kkt, "sums": sums}


def compose(rr, rb, sx, gmax, mu):
    """(primal, dual, gap, scale) from ||r||^2, <r, b>, sum ||x_i||, gmax."""
    scale = type(gmax)(1) if gmax <= mu else mu / gmax
    primal = rr / 2 + mu * sx
    dual = -scale * scale * rr / 2 - scale * rb
    return primal, dual, primal - dual, scale


def certificate(x, A, b, mu):
    """The whole certificate in the dtype of A. Keys as glx.certificate's, plus the raw sums
    "rr" = ||r||^2, "rb" = <r, b>, "sum_xnorm", "kkt_sq" and the arrays "r", "g", "row_norms"."""
    dt = A.dtype
    x = x.astype(dt)
    b = b.astype(dt)
    r = A @ x - b
    g = A.T @ r
    rt = row_terms(x, g, mu)
    sx, gmax, kmax, ksq, nzr = rt["sums"]
    rr, rb = np.sum(r * r), np.sum(r * b)
    primal, dual, gap, scale = compose(rr, rb, sx, gmax, dt.type(mu))
    tiny = np.finfo(np.float64).tiny
    return {"primal": primal, "dual": dual, "gap": gap, "rel_gap": gap / max(abs(primal), tiny),
            "scale": scale, "gmax": gmax, "kkt_max": kmax, "kkt_fro": np.sqrt(ksq),
            "nonzero_rows": int(nzr), "rr": rr, "rb": rb, "sum_xnorm": sx, "kkt_sq": ksq,
            "r": r, "g": g, "row_norms": rt["gnorm"]}


def mu_max(A, b):
    """max_i ||(A^T b)_i||_2: the smallest mu at which x = 0 is optimal."""
    g = A.T @ b
    return np.max(np.sqrt(np.sum(g * g, axis=1)))
