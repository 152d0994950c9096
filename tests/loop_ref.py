"""The loop of the certified solve (solve() in csrc/screen.cpp; DESIGN.md "Certified solve and
screening") in NumPy: the test reference of whole solves, iterate by iterate.

screen_ref.fista_screen and group_ref.fista_screen are references of the fixed point: they restart
adaptively, compact whenever a row goes and check where they please. This model follows the GPU
loop's own rules instead, so that its iterates, counters and screening decisions can be compared
with the GPU's one for one:

  * a check (certificate, stop rule, guard, screen) before the first iteration, then after every
    check_every-th iteration and after iteration maxit;
  * a compaction only when the kept width, padded to a multiple of 64, is at most 0.9 of the current
    width (n at first, a padded width afterwards); it restarts the momentum (y = x, k = 1);
  * kept == 0 ends the solve with x = 0;
  * the returned x holds the rows the last screen listed and +0 elsewhere, whether a compaction
    dropped the others or not;
  * theta = 2 / (k + 1), theta' = 2 / (k + 2), no adaptive restart;
  * a round ends when the reduced problem meets `target`; the full problem's certificate decides,
    and up to five more rounds run with target *= 0.5.

The step is 1 / eigvalsh(A^T W A)[-1] in float64. `dtype` (np.longdouble, np.float64 or np.float32)
is the arithmetic of the iterates: y - t g, the prox, the momentum, and the two products with A. The
certificates of the checks are the trusted references' (certificate_ref, group_ref; sample weights
through sw_ref's reduction to (sqrt(w) o A, sqrt(w) o b)) on the current iterate, in longdouble for
a longdouble run and in float64 otherwise; the guards are screen_ref's, group_ref's and sw_ref's
mirrors with the eps of the GPU's dtype (float32 for a float32 run, float64 otherwise). Imports
nothing from glx.

Two more arms follow solve() in the same way.

The intercept (`ic`; rows or groups, sample weights or ones with sigma = m): the step is
1 / eigvalsh of the centred weighted Gram matrix (ic_ref.centre). An iteration never centres A: p = A y
in T, r^ = p - b in T, the weighted column means of r^ in double (longdouble for a longdouble run),
r_c = T(r^ - mean), r = w o r_c in T, g = A^T r, where k_cert_csum and k_cert_fin_c round. A check is
ic_ref.certificate on the current columns, ic_ref.guard / group_guard on ic_ref.figures with ||b~|| as
solve() forms it, sqrt((||P~ b~||^2 + sigma ||b-bar||^2) (1 + 8 eps)), and the test against
(mu - slack) (1 - 4 eps64). info["intercept"] is ic_ref.intercept_of the returned x.

The sparse-group lasso (`tau` > 0, with groups): the step's prox is the two-level one with k_sgl_fista's
denominators (_prox_sgl). A check is sgl_ref.certificate, the second dual solve (exact_sg on
mul rho + add ||r||, sgl_ref.guard_pad's padding; certificate.cpp hands its unclamped minimum to the
guard, which clamps it at 1), sgl_ref.guard and sgl_ref.keep_rows with a_lo = tau mu (1 - 8 eps64),
cb_lo = (1 - tau) mu (1 - 8 eps64), the group test off at tau = 1. A compaction takes the kept rows,
the groups that keep one, ptr / weights / gcn from sgl_ref.expand_lists (gcn carried over, not
recomputed) and cn gathered. kept and kept_history count groups, kept_row_history rows; min_margin
covers |lhs / a_lo - 1| over the rows and |lhs / cb_lo - 1| over the groups where their test is on.
"""
import functools

import numpy as np

import certificate_ref as cref
import group_ref as gr
import ic_ref as icr
import screen_ref as sr
import sgl_ref as sg
import sw_ref as sw

LD = np.longdouble
MAX_ROUNDS = 6


def pad64(v):
    return (int(v) + 63) // 64 * 64


def step(A, w=None):
    """1 / lambda_max(A^T W A), float64."""
    A = np.asarray(A, dtype=np.float64)
    At = A if w is None else np.sqrt(np.asarray(w, dtype=np.float64))[:, None] * A
    return 1.0 / float(np.linalg.eigvalsh(At.T @ At)[-1])


def _prox_rows(wv, tmu, tiny):
    """fista_row's prox: w max(||w|| - t mu, 0) / ((||w|| < thres) + ||w||)."""
    nrm = np.sqrt(np.sum(wv * wv, axis=1))
    c = np.maximum(nrm - tmu, 0)
    d = (nrm < tiny).astype(wv.dtype) + nrm
    return wv * (c / d)[:, None]


def _prox_groups(wv, tmuw, ptr, tiny):
    """k_group_fista's: the same on the groups' Frobenius norms, t mu w_g per group."""
    nrm = gr.group_norms(wv, ptr)
    c = np.maximum(nrm - tmuw, 0)
    d = (nrm < tiny).astype(wv.dtype) + nrm
    return wv * gr.expand_rows(c / d, ptr)[:, None]


def _prox_sgl(wv, ta, tcw, ptr, tiny):
    """k_sgl_fista's: sgl_ref.prox with the kernel's denominators and order, ((wv c1) / d1 c2) / d2 with
    c1 = (||w_i|| - t a)_+, c2 = (q_g - t c_g)_+, d = (. < thres) + . ; a zero row or group is +0."""
    rho = sg.row_norms(wv)
    c1 = np.maximum(rho - ta, 0)
    d1 = (rho < tiny).astype(wv.dtype) + rho
    q = np.sqrt(np.add.reduceat(c1 * c1, np.asarray(ptr[:-1], dtype=np.intp)))
    c2 = gr.expand_rows(np.maximum(q - tcw, 0), ptr)
    d2 = gr.expand_rows((q < tiny).astype(wv.dtype) + q, ptr)
    uv = (wv * c1[:, None]) / d1[:, None]
    pv = (uv * c2[:, None]) / d2[:, None]
    return np.where(((c1 == 0) | (c2 == 0))[:, None], wv.dtype.type(0), pv)


def run(A, b, mu, x0=None, maxit=100, check_every=10, screen=True, dtype=np.float64, ptr=None, w=None, tol=1e-30,
        gw=None, snap=(), ic=False, tau=0.0):
    """The certified solve's loop on (A, b) (float64 arrays: what the GPU is given, already rounded
    where it works in float32) at mu. ptr / gw: group_ptr and the groups' weights (None: rows);
    w: sample weights (None: unweighted). Returns (x (n x l) in `dtype`, info): iterations, checks,
    compactions, kept_history (rows, or groups, kept at each compaction), kept (at the last screen; n
    or G without one), kept_rows (ascending indices of the rows not proven zero), kept_groups, width,
    rounds, converged, rel_gap (the full problem's, of the returned x), step, and min_margin: the
    smallest |lhs_i / mu_lo - 1| over all rows (groups) at all screens, lhs_i = s rn_i + cn_i rho, the
    distance of the closest screening decision from its threshold. snap: iteration numbers after which
    the iterate (scattered to n x l) is copied into info["snapshots"][it]: with screening off the
    iterates do not depend on maxit, so one run serves several. ic: the problem with an unpenalised
    intercept (info["intercept"]: the returned x's, longdouble); tau > 0 (with ptr / gw): the sparse-group
    lasso (info["kept_row_history"]: rows kept at each compaction). The module docstring has both."""
    T = np.dtype(dtype).type
    wide = LD if T is LD else np.float64
    eps = sr.EPS32 if T is np.float32 else sr.EPS64
    tiny = T(np.finfo(np.float32 if T is np.float32 else np.float64).tiny)
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    m, n = A.shape
    l = b.shape[1]
    grouped = ptr is not None
    if grouped:
        ptr = np.asarray(ptr)
        gw = np.asarray(gw, dtype=np.float64)
    sgl = grouped and float(tau) > 0.0
    tau = float(tau)
    if ic:
        # weights of one stand for none (sigma = m); the pair of the step is the centred one, never the GPU's
        w1 = np.ones(m) if w is None else np.asarray(w, dtype=np.float64)
        Acen = icr.centre(A, b, w1)[0]
        t = 1.0 / float(np.linalg.eigvalsh(Acen.T @ Acen)[-1])
        At, bt = A, b               # (the certificates centre the current columns themselves)
        cn_ld = icr.col_norms(A, w1)
        cn_all = np.asarray(cn_ld, dtype=np.float64)
        cstats, _, sigma = icr.figures(A, b, w1)
        bbar = icr.col_means(b, w1)
        bcen = icr.centre(A, b, w1, LD)[1]
        # solve(): bn = sqrt((h[0] + sigma mean_sq) (1 + 8 eps)), h[0] = ||P~ b~||^2, the means -b-bar
        bn = float(np.sqrt((float(np.sum(bcen * bcen)) + sigma * float(np.sum(bbar * bbar))) * (1.0 + 8.0 * sr.EPS64)))
        csq = cstats[1]
        if grouped:
            G = ptr.size - 1
            gcn_all = np.asarray(np.sqrt(np.add.reduceat(cn_ld * cn_ld, np.asarray(ptr[:-1], dtype=np.intp)))
                                 / gw.astype(LD), dtype=np.float64)
            max_run, w_min, gcmax = int(np.diff(ptr).max()), float(gw.min()), float(gcn_all.max())
    else:
        t = step(A, w)
        # the certificates' pair: the reduction of the weighted problem, in `wide`
        At, bt = (A.astype(wide), b.astype(wide)) if w is None else sw.reduce(A, b, w, wide)
        cn_all = np.asarray(sr.col_norms(At), dtype=np.float64)
        csq, bn = float(np.sum(cn_all ** 2)), float(np.sqrt(np.sum(bt * bt)))
        if grouped:
            G = ptr.size - 1
            gcn_all = np.asarray(gr.group_cnorms(At, ptr, gw), dtype=np.float64)
            max_run, w_min, gcmax = int(np.diff(ptr).max()), float(gw.min()), float(gcn_all.max())
        if sgl or not grouped:
            cmax = float(cn_all.max())
    mu_lo = mu * (1.0 - 4.0 * sr.EPS64)
    # the iterates' operands, in T
    AT, bT = A.astype(T), b.astype(T)
    wT = None if w is None else np.asarray(w, dtype=np.float64).astype(T)[:, None]
    tT, tmuT = T(t), T(float(t) * float(mu))
    if ic:      # the means' arithmetic: double on the GPU whatever T is
        D = LD if T is LD else np.float64
        wD, sigD = w1.astype(D), D(sigma)
    if sgl:     # t a and t (1 - tau) mu: double products rounded to T, as launch_sgl_fista passes them
        taT, tcT = T(float(t) * (tau * float(mu))), T(float(t) * ((1.0 - tau) * float(mu)))
        shave = 1.0 - 8.0 * sr.EPS64
        a_lo, cb_lo = tau * mu * shave, (1.0 - tau) * mu * shave

    st = {"rows": np.arange(n), "gidx": np.arange(G) if grouped else None, "pc": ptr, "gwc": gw,
          "Ac": AT, "Atc": At, "wc": n, "k": 1, "it": 0, "all_zero": False, "target": float(tol),
          "kept": G if grouped else n, "last": None, "listed": None}
    if sgl:
        st["cn"], st["gcn"] = cn_all, gcn_all
    x = np.zeros((n, l), dtype=T) if x0 is None else np.array(x0, dtype=np.float64).astype(T)
    st["x"], st["y"] = x, x.copy()
    info = {"checks": 0, "compactions": 0, "kept_history": [], "min_margin": np.inf, "snapshots": {}}
    if sgl:
        info["kept_row_history"], info["group_row_history"] = [], []

    def certificate(xx, Atc, pc, gwc):
        if ic:
            return icr.certificate(xx, Atc, b, mu, w1, pc, gwc, wide)
        if sgl:
            return sg.certificate(xx.astype(wide), Atc, bt, wide(mu), pc, gwc, tau)
        if grouped:
            return gr.certificate(xx.astype(wide), Atc, bt, wide(mu), pc, gwc)
        return cref.certificate(xx.astype(wide), Atc, bt, wide(mu))

    def check_sgl(c, met):
        """The sparse-group screen and compaction of one check (the tail of check())."""
        wc, pc, gwc, cn, gcn = st["wc"], st["pc"], st["gwc"], st["cn"], st["gcn"]
        weighted = w is not None
        rec = [float(c["rr"]), float(c["rb"]), float(c["omega"])]
        rho = np.asarray(c["row_norms"], dtype=np.float64)      # (the kernels work on n doubles)
        # the second dual solve on p_i = mul rho_i + add ||r||; its unclamped minimum goes to the guard
        mul, addc = sg.guard_pad(eps, m, l, max_run, cmax, weighted)
        p = mul * rho + addc * np.sqrt(rec[0])
        s_pad = float(np.min(sg.exact_sg(p, pc, gwc, tau * mu, (1.0 - tau) * mu)))
        mul, add, s, _, rad = sg.guard(rec, s_pad, mu, tau, eps, m, wc, l, max_run, w_min, cmax, csq, bn, weighted)
        keep, galive = sg.keep_rows(rho, cn, gcn, pc, gwc, s, mul, add, rad, a_lo, cb_lo, tau < 1.0)
        pl = LD(mul) * rho.astype(LD) + LD(add)
        marg = np.abs((LD(s) * pl + cn.astype(LD) * LD(rad)) / LD(a_lo) - 1)
        if tau < 1.0:
            v = np.maximum(LD(s) * pl - LD(a_lo), 0)
            ph = np.sqrt(np.add.reduceat(v * v, np.asarray(pc[:-1], dtype=np.intp)))
            marg = np.concatenate((marg, np.abs((ph / gwc.astype(LD) + gcn.astype(LD) * LD(rad)) / LD(cb_lo) - 1)))
        info["min_margin"] = min(info["min_margin"], float(np.min(marg)))
        kept, krows = int(galive.sum()), int(keep.sum())
        wp = pad64(krows)
        st["kept"] = kept
        st["last"] = (st["rows"][keep], st["gidx"][galive])
        st["listed"] = keep
        if met or wp * 10 > wc * 9:
            return met
        st["listed"] = None
        info["kept_history"].append(kept)
        info["kept_row_history"].append(krows)
        info["group_row_history"].append(int(np.diff(pc)[galive].sum()))    # (rows of the groups that survive)
        info["compactions"] += 1
        if kept == 0:
            st["all_zero"] = True
            st["wc"] = 0
            return True
        _, nptr, nw, ngcn, gm, _ = sg.expand_lists(keep, pc, gwc, gcn, st["gidx"])
        st["pc"], st["gwc"], st["gcn"], st["gidx"] = nptr, nw, ngcn, np.asarray(gm, dtype=np.int64)
        st["cn"] = cn[keep]
        st["rows"], st["Ac"], st["Atc"], st["x"] = st["rows"][keep], st["Ac"][:, keep], st["Atc"][:, keep], st["x"][keep]
        st["y"], st["k"] = st["x"].copy(), 1
        st["wc"] = wp
        return False

    def check():
        info["checks"] += 1
        c = certificate(st["x"], st["Atc"], st["pc"], st["gwc"])
        met = float(c["rel_gap"]) <= st["target"]
        if not screen:
            return met
        if sgl:
            return check_sgl(c, met)
        wc = st["wc"]
        lo = mu_lo
        if ic:      # the guards of the intercept: the slack comes off mu
            msq = float(np.sum(np.asarray(c["intercept"], dtype=np.float64) ** 2))
            if grouped:
                s, _, rho, slack = icr.group_guard(gr.record(c), mu, eps, m, wc, l, max_run, w_min, gcmax, cstats, bn,
                                                   sigma, msq)
                rn, cn = c["group_norms"], gcn_all[st["gidx"]]
            else:
                s, _, rho, slack = icr.guard(sr.record(c), mu, eps, m, wc, l, cstats, bn, sigma, msq)
                rn, cn = c["row_norms"], cn_all[st["rows"]]
            lo = (mu - slack) * (1.0 - 4.0 * sr.EPS64)
        elif grouped:
            g_ = gr.guard if w is None else sw.group_guard
            s, _, rho = g_(gr.record(c), mu, eps, m, wc, l, max_run, w_min, gcmax, csq, bn)
            rn, cn = c["group_norms"], gcn_all[st["gidx"]]
        else:
            g_ = sr.guard if w is None else sw.guard
            s, _, rho = g_(sr.record(c), mu, eps, m, wc, l, cmax, csq, bn)
            rn, cn = c["row_norms"], cn_all[st["rows"]]
        lhs = LD(s) * rn.astype(LD) + cn.astype(LD) * LD(rho)
        with np.errstate(invalid="ignore"):
            keep = ~(lhs < LD(lo))
        info["min_margin"] = min(info["min_margin"], float(np.min(np.abs(lhs / LD(lo) - 1))))
        rk = gr.expand_rows(keep, st["pc"]) if grouped else keep
        kept, wp = int(keep.sum()), pad64(int(rk.sum()))
        st["kept"] = kept
        st["last"] = (st["rows"][rk], st["gidx"][keep] if grouped else None)
        st["listed"] = rk          # (the rows of the current problem the screen listed; None once compacted)
        if met or wp * 10 > wc * 9:
            return met
        st["listed"] = None
        info["kept_history"].append(kept)
        info["compactions"] += 1
        if kept == 0:
            st["all_zero"] = True
            st["wc"] = 0
            return True
        if grouped:
            st["pc"] = np.concatenate(([0], np.cumsum(np.diff(st["pc"])[keep])))
            st["gidx"], st["gwc"] = st["gidx"][keep], st["gwc"][keep]
        st["rows"], st["Ac"], st["Atc"], st["x"] = st["rows"][rk], st["Ac"][:, rk], st["Atc"][:, rk], st["x"][rk]
        st["y"], st["k"] = st["x"].copy(), 1      # the momentum restarts
        st["wc"] = wp
        return False

    def iterate():
        k = st["k"]
        theta, a1, b1 = T(2.0 / (k + 1)), T(1.0 - 2.0 / (k + 2)), T(2.0 / (k + 2))
        xk, y, Ac = st["x"], st["y"], st["Ac"]
        r = Ac @ y - bT
        if ic:      # k_cert_csum, k_cert_fin_c: the means in double, r_c rounded to T, then the weight
            mean = (wD @ r.astype(D)) / sigD
            r = (r.astype(D) - mean[None, :]).astype(T)
        if wT is not None:
            r = wT * r
        g = Ac.T @ r
        wv = y - tT * g
        if sgl:
            xc = _prox_sgl(wv, taT, tcT * st["gwc"].astype(T), st["pc"], tiny)
        elif grouped:
            xc = _prox_groups(wv, tmuT * st["gwc"].astype(T), st["pc"], tiny)
        else:
            xc = _prox_rows(wv, tmuT, tiny)
        xo = np.where(np.abs(xk) < tiny, T(0), xk)
        vn = xo + (xc - xo) / theta
        st["y"] = a1 * np.where(np.abs(xc) < tiny, T(0), xc) + b1 * vn
        st["x"] = xc
        st["k"] += 1
        st["it"] += 1
        if st["it"] in snap:
            X = np.zeros((n, l), dtype=T)
            X[st["rows"]] = st["x"]
            info["snapshots"][st["it"]] = X

    def full():
        X = np.zeros((n, l), dtype=T)
        if not st["all_zero"]:        # where the last check screened without compacting, its rows alone
            rk = slice(None) if st["listed"] is None else st["listed"]
            X[st["rows"][rk]] = st["x"][rk]
        c = certificate(X, At, ptr, gw)
        return X, float(c["rel_gap"])

    converged = False
    for rnd in range(MAX_ROUNDS):
        info["rounds"] = rnd + 1
        met = check()
        while not met and not st["all_zero"] and st["it"] < maxit:
            iterate()
            if st["it"] % check_every == 0 or st["it"] >= maxit:
                met = check()
        X, rel = full()
        if rel <= tol:
            converged = True
            break
        if st["it"] >= maxit or st["all_zero"]:
            break
        st["target"] *= 0.5

    if st["last"] is None:      # no screen ran: nothing is proven
        kept_rows, kept_groups = np.arange(n), (np.arange(G) if grouped else None)
    else:
        kept_rows, kept_groups = st["last"]
    info.update(iterations=st["it"], kept=st["kept"], kept_rows=np.asarray(kept_rows, dtype=np.int64),
                kept_groups=kept_groups, width=st["wc"], converged=converged, rel_gap=rel, step=t)
    if ic:
        info["intercept"] = icr.intercept_of(X, A, b, w1, LD)
    return X, info


# ------------------------------------------------------------------------------------------ shared cases
SEED = 1            # the gen_data seed of the screen tests
X0_SEED = 5


@functools.lru_cache(maxsize=None)
def problem(kind, m, n, l, ratio, f32=False, pool=None, tau=None, wkind=None):
    """The instances of the loop tests at mu = ratio * mu_max, float64 arrays (read-only, shared):
    "rows" = glx.driver.gen_data(SEED, m, n, l); "sw" = the same with sw_ref's general sample weights
    (a quarter of them zero); "grp" = group_ref.instance(group_ref.SEED, m, n, l, pool). f32: A, b and
    the weights rounded to float32 first, the instance a float32 solve sees.
    "ic" / "icg" = ic_ref.offset_instance(m, n, l) with an intercept ("ic": True), rows or the groups and
    group weights of ic_ref.group_reference_solution, with the sample weights sw_ref.weights_of(wkind, m)
    (wkind None: none), at ratio times the intercept problem's mu_max (float64, as the references take it).
    "sgl" = sgl_ref.instance(sgl_ref.SEED, m, n, l, pool) at the row ratio tau ("tau"), sample weights by
    wkind, at ratio times sgl_ref.mu_max (of the reduced pair with weights)."""
    ptr = gw = w = None
    if kind == "grp":
        A, b, ptr, gw = gr.instance(gr.SEED, m, n, l, pool)
    elif kind in ("ic", "icg"):
        A, b = icr.offset_instance(m, n, l)
        if kind == "icg":
            ptr = gr.draw_groups(np.random.default_rng(sw.WSEED + 2), n, sw.GROUP_SIZES)
            gw = np.sqrt(np.diff(ptr).astype(np.float64))
    elif kind == "sgl":
        A, b, ptr, gw = sg.instance(sg.SEED, m, n, l, pool)
    else:
        A, b, _, _ = cref.instance(SEED, m, n, l)
        if kind == "sw":
            w = sw.weights_of("general", m)
    if wkind is not None:
        w = sw.weights_of(wkind, m)
    if f32:
        A, b, gw, w = (None if a is None else a.astype(np.float32).astype(np.float64) for a in (A, b, gw, w))
    if kind == "grp":
        top = gr.mu_max(A, b, ptr, gw)
    elif kind in ("ic", "icg"):
        top = float(icr.mu_max(A, b, np.ones(m) if w is None else w, ptr, gw, wide=np.float64))
    elif kind == "sgl":
        At, bt = (A, b) if w is None else sw.reduce(A, b, w)
        top = sg.mu_max(At, bt, ptr, gw, tau)
    else:
        top = float(cref.mu_max(A, b)) if w is None else float(sw.mu_max(A, b, w, wide=np.float64))
    for a in (A, b, ptr, gw, w):
        if a is not None:
            a.setflags(write=False)
    out = {"A": A, "b": b, "mu": float(ratio) * top, "ptr": ptr, "gw": gw, "w": w}
    if kind in ("ic", "icg"):
        out["ic"] = True
    if kind == "sgl":
        out["tau"] = float(tau)
    return out


@functools.lru_cache(maxsize=None)
def start(n, l, scale, f32=False):
    """The random nonzero x0 of the loop tests: scale * standard normals (seeded), read-only."""
    x0 = float(scale) * np.random.default_rng(X0_SEED).standard_normal((n, l))
    if f32:
        x0 = x0.astype(np.float32).astype(np.float64)
    x0.setflags(write=False)
    return x0


@functools.lru_cache(maxsize=None)
def model(pkey, dtype, maxit, check_every=10, screen=True, x0_scale=None, snap=(), tol=1e-30):
    """run() on problem(*pkey), computed once per argument tuple and shared (do not modify the result).
    dtype: "ld", "f64" or "f32"; x0_scale: None = x0 = 0, else start(n, l, x0_scale)."""
    p = problem(*pkey)
    n, l = p["A"].shape[1], p["b"].shape[1]
    f32 = len(pkey) > 5 and bool(pkey[5])
    x0 = None if x0_scale is None else start(n, l, x0_scale, f32)
    T = {"ld": LD, "f64": np.float64, "f32": np.float32}[dtype]
    return run(p["A"], p["b"], p["mu"], x0, maxit, check_every, screen, T, ptr=p["ptr"], w=p["w"], tol=tol,
               gw=p["gw"], snap=tuple(snap), ic=p.get("ic", False), tau=p.get("tau", 0.0))


def x_bar(x_T, x_ld, eps):
    """The bar of a GPU iterate against the longdouble model's: 16 d + 4 eps max |x_LD| with
    d = max |x_T - x_LD|, the distance of the model run in the working dtype from the longdouble one
    (what rounding alone does to this trajectory in NumPy's order of operations; the factor 16 is a
    margin for the GPU's different summation orders, a supposition)."""
    d = float(np.max(np.abs(x_T.astype(LD) - x_ld)))
    return 16.0 * d + 4.0 * eps * float(np.max(np.abs(x_ld)))


# (name, problem key, maxit, check_every, x0 scale, the model's kept_history): what
# tests/test_loop_ref_cpu.py pins and tests/test_gpu_certified_loop.py compares the GPU loop with.
# Widths of the first: 512 -> 384 -> 128 -> 64, a third compaction (every two-buffer ping-pong is
# back on its first side). "ce=3" compacts at its final check (iteration 20) as well.
LOOP_CASES = [
    ("96x512x16@0.5", ("rows", 96, 512, 16, 0.5), 45, 10, None, [376, 82, 54]),
    ("40x200x3@0.3", ("rows", 40, 200, 3, 0.3), 45, 10, None, [101, 38]),
    ("40x200x3@0.3-ce=3", ("rows", 40, 200, 3, 0.3), 20, 3, None, [127, 49]),
    ("64x1024x16@0.5", ("rows", 64, 1024, 16, 0.5), 45, 10, None, [814]),
    ("groups", ("grp", 96, 512, 16, 0.5, False, gr.POOL_SMALL), 45, 10, None, [27, 13]),
    ("sample weights", ("sw", 96, 512, 16, 0.5), 45, 10, None, [237, 143]),
    # the intercept: general sample weights, none, check_every = 3 (the row kernel's shape), groups
    ("ic weights", ("ic", 96, 512, 16, 0.5, False, None, None, "general"), 45, 10, None, [422, 197, 115]),
    ("ic", ("ic", 96, 512, 16, 0.5), 45, 10, None, [428, 86, 54]),
    ("ic ce=3", ("ic", 40, 200, 3, 0.5, False, None, None, "general"), 20, 3, None, [68, 50]),
    ("ic groups", ("icg", 96, 512, 16, 0.7, False, None, None, "general"), 45, 10, None, [63, 37, 34]),
    # the sparse-group lasso (kept_history counts groups; the rows are in ROW_HISTORIES)
    # (tau = 0.3: the second compaction drops 20 groups and one interior row of a group that stays)
    ("sgl tau=0.3", ("sgl", 40, 200, 3, 0.5, False, gr.POOL_SMALL, 0.3), 45, 10, None, [25, 5]),
    ("sgl tau=0.3 l=16", ("sgl", 96, 512, 16, 0.5, False, gr.POOL_SMALL, 0.3), 45, 10, None, [22, 12]),
    ("sgl tau=0.9 long", ("sgl", 96, 512, 16, 0.5, False, gr.POOL_LONG, 0.9), 45, 10, None, [15, 1]),
    ("sgl tau=1", ("sgl", 96, 512, 16, 0.5, False, gr.POOL_SMALL, 1.0), 45, 10, None, [89, 25]),
    ("sgl weights", ("sgl", 96, 512, 16, 0.5, False, gr.POOL_SMALL, 0.3, "general"), 45, 10, None, [24, 19]),
    ("sgl ce=3", ("sgl", 40, 200, 3, 0.5, False, gr.POOL_RAGGED, 0.3), 20, 3, None, [30, 14]),
]
BRANCH_CASES = [
    ("ce=1", ("rows", 40, 200, 3, 0.3), 20, 1, None, [127, 63]),
    ("ce=7", ("rows", 40, 200, 3, 0.3), 20, 7, None, [101]),
    ("ce=maxit+5", ("rows", 40, 200, 3, 0.3), 20, 25, None, [101]),
    # mu = 1.05 mu_max from a random x0: every row is proven zero while the iterate is not yet zero
    ("kept=0", ("rows", 96, 512, 16, 1.05), 500, 10, 1.0, [0]),
    ("kept=0-ce=1", ("rows", 96, 512, 16, 1.05), 500, 1, 1.0, [75, 4, 0]),
    # the same branch with an intercept (no weights) and in the sparse-group arm (after a compaction)
    ("ic kept=0", ("ic", 96, 512, 16, 1.05), 500, 10, 1.0, [0]),
    ("ic kept=0-ce=1", ("ic", 96, 512, 16, 1.05), 500, 1, 1.0, [122, 5, 0]),
    ("sgl kept=0", ("sgl", 96, 512, 16, 1.05, False, gr.POOL_RAGGED, 0.3), 500, 2, 1.0, [4, 0]),
]
# the sparse-group cases' kept_row_history, by name (rows after each compaction, beside the groups above)
ROW_HISTORIES = {
    "sgl tau=0.3": [107, 14], "sgl tau=0.3 l=16": [72, 47], "sgl tau=0.9 long": [322, 41], "sgl tau=1": [179, 47], "sgl weights": [82, 57],
    "sgl ce=3": [103, 43], "sgl kept=0": [16, 0],
}
