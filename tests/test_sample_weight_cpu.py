"""Sample weights and cross-validation without a device (DESIGN.md "Sample weights and
cross-validation"): the argument checks that must raise before any device call, the fold helper and
the aggregate against hand-computed values, the two weighted guards against their mirrors
(tests/sw_ref.py) and the safety of the guarded test at the reference solutions of the weighted
instances the GPU tests solve, also with the record's gap forced to 0 and below.
"""
import numpy as np
import pytest

import group_ref as gr
import screen_ref as sr
import sw_ref as sw


# ------------------------------------------------------------------------------------------ arguments
def test_check_sample_weight():
    from glx.certificate import check_sample_weight
    assert check_sample_weight(None, 5) is None
    w = check_sample_weight([0, 1, 2.5], 3)
    assert w.dtype == np.float64 and w.flags.c_contiguous and np.array_equal(w, [0, 1, 2.5])
    w32 = check_sample_weight(np.array([1.0, 1.0 + 2.0 ** -30]), 2, np.float32)
    assert w32.dtype == np.float32 and np.array_equal(w32, [1.0, 1.0])      # rounded once, on the host
    for bad in ([1.0, 2.0], [[1.0, 2.0, 3.0]], [1.0, -1e-300, 1.0], [1.0, np.nan, 1.0], [1.0, np.inf, 1.0],
                [0.0, 0.0, 0.0]):
        with pytest.raises(ValueError):
            check_sample_weight(bad, 3)
    with pytest.raises(ValueError):         # finite in float64, infinite once rounded to A's dtype
        check_sample_weight([1.0, 1e300, 1.0], 3, np.float32)
    with pytest.raises(ValueError):         # positive in float64, all zero once rounded
        check_sample_weight([0.0, 1e-300, 0.0], 3, np.float32)


def test_weighted_entries_refuse_before_any_device_work():
    """This machine may have no GPU: every call below must raise ValueError from the host checks."""
    import glx
    A, b = np.ones((4, 6)), np.ones((4, 2))
    x = np.zeros((6, 2))
    bads = ([1.0, 1.0, 1.0], [1.0, -1.0, 1.0, 1.0], [1.0, np.nan, 1.0, 1.0], [1.0, np.inf, 1.0, 1.0], [0.0] * 4)
    for bad in bads:
        with pytest.raises(ValueError):
            glx.certificate(x, A, b, 0.1, sample_weight=bad)
        with pytest.raises(ValueError):
            glx.mu_max(A, b, sample_weight=bad)
        with pytest.raises(ValueError):
            glx.solve_certified(A, b, 0.1, sample_weight=bad)
        with pytest.raises(ValueError):
            glx.solve_certified(A, b, 0.1, sample_weight=np.ones(4), holdout_weight=bad)
        with pytest.raises(ValueError):
            glx.path(A, b, sample_weight=bad)
        with pytest.raises(ValueError):
            glx.cv_path(A, b, folds=2, sample_weight=bad)
    with pytest.raises(ValueError):
        glx.solve_certified(A, b, 0.1, sample_weight=np.ones(4), groups=[0, 3, 5])   # the groups' own check
    for folds in (1, 5, np.array([0, 0, 0, 0]), np.array([0, 2, 0, 2]), np.array([0, 1, 0]), np.array([0.0, 1, 0, 1]),
                  np.array([0, -1, 0, 1])):
        with pytest.raises(ValueError):
            glx.cv_path(A, b, folds=folds)
    with pytest.raises(ValueError):         # the sample weights leave fold 1 without held-out mass
        glx.cv_path(A, b, folds=2, sample_weight=[1.0, 0.0, 1.0, 0.0])
    with pytest.raises(ValueError):
        glx.cv_path(A, b, folds=2, mus=[1.0, 2.0])
    with pytest.raises(ValueError):
        glx.cv_path(A, b, folds=2, tol=0.0)


# ------------------------------------------------------------------------------------------ folds
def test_fold_helpers_by_hand():
    from glx.cv import fold_labels, fold_weights
    lab, K = fold_labels(3, 7)
    assert K == 3 and np.array_equal(lab, [0, 1, 2, 0, 1, 2, 0])
    lab2, K2 = fold_labels(np.array([2, 0, 1, 1, 0, 2, 2]), 7)
    assert K2 == 3 and np.array_equal(lab2, [2, 0, 1, 1, 0, 2, 2])
    tr, ho = fold_weights(lab, 1)
    assert np.array_equal(tr, [1, 0, 1, 1, 0, 1, 1]) and np.array_equal(ho, [0, 1, 0, 0, 1, 0, 0])
    w = np.array([0.5, 2.0, 0.0, 3.0, 1.0, 1.0, 4.0])
    tr, ho = fold_weights(lab, 0, w, np.float32)
    assert tr.dtype == np.float32 and np.array_equal(tr, [0, 2, 0, 0, 1, 1, 0]) and np.array_equal(ho, [0.5, 0, 0, 3, 0, 0, 4])
    for k in range(3):
        a, c = fold_weights(lab, k, w)
        r1, r2 = sw.fold_vectors(lab, k, w)
        assert np.array_equal(a, r1) and np.array_equal(c, r2) and np.array_equal(a + c, w)
    with pytest.raises(ValueError):         # the only row of fold 2 weighs 0: nothing is held out
        fold_weights(np.array([0, 1, 2]), 2, np.array([1.0, 1.0, 0.0]))


def test_aggregate_by_hand():
    from glx.cv import aggregate
    fl = np.array([[4.0, 2.0, 1.0, 3.0],
                   [6.0, 2.0, 3.0, 3.0],
                   [5.0, 5.0, 2.0, 6.0]])
    out = aggregate(fl, [8.0, 4.0, 2.0, 1.0])
    assert np.array_equal(out["mean"], [5.0, 3.0, 2.0, 4.0])
    # se = sqrt(sum (v - mean)^2 / (K - 1) / K): [sqrt(2/6), sqrt(6/6), sqrt(2/6), sqrt(6/6)]
    assert np.allclose(out["se"], [np.sqrt(1 / 3), 1.0, np.sqrt(1 / 3), 1.0], rtol=4 * sr.EPS64, atol=0)
    assert out["best"] == 2 and out["one_se"] == 2          # 3.0 > 2 + 0.577
    assert out["mu_best"] == 2.0 and out["mu_one_se"] == 2.0
    mean, se, best, one = sw.cv_aggregate(fl)
    assert np.allclose(out["mean"], mean, rtol=4 * sr.EPS64) and np.allclose(out["se"], se, rtol=8 * sr.EPS64)
    assert (best, one) == (2, 2)
    # the minimum at the small-mu end; the one-standard-error rule walks back to the largest mu within it
    fl2 = np.array([[9.0, 3.2, 3.1, 2.0], [9.0, 2.8, 2.9, 4.0]])
    out2 = aggregate(fl2, [4.0, 3.0, 2.0, 1.0])
    assert out2["best"] == 1 and np.array_equal(out2["mean"], [9.0, 3.0, 3.0, 3.0])   # the first of the ties
    fl3 = np.array([[9.0, 5.0, 3.5, 2.0], [9.0, 5.0, 3.5, 4.0]])
    out3 = aggregate(fl3, [4.0, 3.0, 2.0, 1.0])
    assert out3["best"] == 3 and out3["se"][3] == 1.0 and out3["one_se"] == 2 and out3["mu_one_se"] == 2.0
    # the minimum at the large-mu end: both indices are 0
    out4 = aggregate(fl3[:, ::-1], [4.0, 3.0, 2.0, 1.0])
    assert out4["best"] == 0 and out4["one_se"] == 0
    with pytest.raises(ValueError):
        aggregate(fl[:1], [8.0, 4.0, 2.0, 1.0])
    with pytest.raises(ValueError):
        aggregate(fl, [8.0, 4.0])


def test_cv_table_has_one_line_per_mu_and_one_best_marker():
    from glx.cv import aggregate, format_table
    fl = np.array([[4.0, 2.0, 1.0, 3.0], [6.0, 2.0, 3.0, 3.0], [5.0, 5.0, 2.0, 6.0]])
    cv = {"mus": [8.0, 4.0, 2.0, 1.0], **aggregate(fl, [8.0, 4.0, 2.0, 1.0])}
    lines = format_table(cv).splitlines()
    assert len(lines) == 5 and sum("best" in ln for ln in lines) == 1 and sum("1-SE" in ln for ln in lines) == 1


# ------------------------------------------------------------------------------------------ guards
def test_weighted_guards_equal_their_mirrors():
    from glx import _lib, kernels as k
    g = np.random.default_rng(17)
    for dtype, eps in ((_lib.GLX_F64, sr.EPS64), (_lib.GLX_F32, sr.EPS32)):
        for _ in range(50):
            m, n, l = int(g.integers(1, 5000)), int(g.integers(1, 20000)), int(g.integers(1, 129))
            rr = float(g.uniform(0.0, 10.0)) * float(g.choice([0.0, 1e-12, 1.0]))
            bn = float(g.uniform(0.0, 10.0))
            rb = float(g.uniform(-1.0, 1.0)) * np.sqrt(rr) * bn
            sx = float(g.uniform(0.0, 50.0))
            gmax = float(g.uniform(0.0, 2.0))
            mu = float(g.choice([0.0, 1e-3, 1.0, 5.0]))
            cmax = float(g.uniform(0.1, 100.0))
            csq = cmax * cmax * float(g.uniform(1.0, n))
            rec = [rr, rb, sx, gmax, 0.0, 0.0, 0.0, 0.0]
            want = sw.guard(rec, mu, eps, m, n, l, cmax, csq, bn)
            got = k.screen_guard_sw(rec, mu, dtype, m, n, l, cmax, csq, bn)
            for a, v in zip(want, got):
                assert abs(v - a) <= 8 * sr.EPS64 * abs(a), (dtype, m, n, l, rec, mu, want, got)
            # one more rounding in the A^T pass: the weighted scale is never the larger one
            assert got[0] <= k.screen_guard(rec, mu, dtype, m, n, l, cmax, csq, bn)[0]
            max_run = int(g.integers(1, min(n, 70) + 1))
            w_min = float(g.uniform(0.1, 3.0))
            want = sw.group_guard(rec, mu, eps, m, n, l, max_run, w_min, cmax, csq, bn)
            got = k.group_screen_guard_sw(rec, mu, dtype, m, n, l, max_run, w_min, cmax, csq, bn)
            for a, v in zip(want, got):
                assert abs(v - a) <= 8 * sr.EPS64 * abs(a), (dtype, m, n, l, max_run, rec, mu, want, got)
            assert got[0] <= k.group_screen_guard(rec, mu, dtype, m, n, l, max_run, w_min, cmax, csq, bn)[0]
    with pytest.raises(_lib.GlxError):
        k.screen_guard_sw([1.0] * 8, -1.0, _lib.GLX_F64, 10, 10, 2, 1.0, 10.0, 1.0)
    with pytest.raises(_lib.GlxError):
        k.group_screen_guard_sw([1.0] * 8, 0.1, _lib.GLX_F64, 10, 10, 2, 11, 1.0, 1.0, 10.0, 1.0)
    out = k.screen_guard_sw([float("nan"), 0.0, 1.0, 1.0, 0, 0, 0, 0], 0.1, _lib.GLX_F64, 10, 10, 2, 1.0, 10.0, 1.0)
    assert all(np.isnan(v) for v in out[1:])


ROW_CASES = [(96, 512, 16, 0.5, "general"), (96, 512, 16, 0.1, "general"), (40, 130, 3, 0.5, "general"),
             (40, 130, 3, 0.1, "general"), (40, 130, 3, 0.1, "mask"), (40, 130, 3, 0.1, "int")]


def _row_case(case):
    from glx import _lib
    m, n, l, ratio, kind = case
    ref = sw.reference_solution(m, n, l, ratio, kind)
    A, b, w, mu, x = ref["A"], ref["b"], ref["w"], ref["mu"], ref["x"]
    c = sw.certificate(x, A, b, mu, w, wide=np.float64)
    cn = np.asarray(sw.col_norms(A, w), dtype=np.float64)
    fig = (float(cn.max()), float(np.sum(cn * cn)), float(np.sqrt(np.sum(w[:, None] * b * b))))
    nz = np.sqrt(np.sum(x * x, axis=1)) != 0
    assert 0 < nz.sum() < n
    return {"m": m, "n": n, "l": l, "mu": mu, "c": c, "cn": cn, "fig": fig, "nz": nz, "dtype": _lib.GLX_F64}


def _row_screened(cs, rec):
    from glx import kernels as k
    s, gap_p, rho = k.screen_guard_sw(rec, cs["mu"], cs["dtype"], cs["m"], cs["n"], cs["l"], *cs["fig"])
    keep = sr.keep_mask(cs["c"]["row_norms"], cs["cn"], s, rho, cs["mu"])
    return s, gap_p, rho, ~keep


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: "%dx%dx%d@%g-%s" % c)
@pytest.mark.parametrize("forced", [None, 0.0, -1e-9], ids=["as-is", "gap0", "gap-1e-9P"])
def test_weighted_guard_is_safe_at_xstar(case, forced):
    cs = _row_case(case)
    rec = sr.record(cs["c"])
    s0, gap_p, rho, scr = _row_screened(cs, rec)
    if forced is None:
        assert rho > 0.0 and gap_p >= max(float(cs["c"]["gap"]), 0.0) and 0.0 < s0 <= 1.0
        assert scr.sum() > 0                     # (x* is accurate enough to screen something)
    else:
        rr, rb, mu = rec[0], rec[1], cs["mu"]
        primal = 0.5 * rr + mu * rec[2]
        rec[2] = (forced * primal - (0.5 * (1.0 + s0 * s0) * rr + s0 * rb)) / mu
        s, gap_p, rho, scr = _row_screened(cs, rec)
        assert s == s0 and rho > 0.0 and gap_p > 0.0
    assert not np.any(scr & cs["nz"])


@pytest.mark.parametrize("forced", [None, 0.0, -1e-9], ids=["as-is", "gap0", "gap-1e-9P"])
def test_weighted_group_guard_is_safe_at_xstar(forced):
    from glx import _lib, kernels as k
    m, n, l, ratio = 96, 512, 16, 0.5
    ref = sw.group_reference_solution(m, n, l, ratio)
    A, b, w, ptr, gw, mu, x = (ref[key] for key in ("A", "b", "w", "ptr", "gw", "mu", "x"))
    c = sw.certificate(x, A, b, mu, w, ptr, gw, wide=np.float64)
    At, _ = sw.reduce(A, b, w)
    gcn = np.asarray(gr.group_cnorms(At, ptr, gw), dtype=np.float64)
    csq, bn = float(np.sum(At * At)), float(np.sqrt(np.sum(w[:, None] * b * b)))
    nz = gr.group_norms(x, ptr) != 0
    assert 0 < nz.sum() < nz.size
    rec = gr.record(c)
    args = (mu, _lib.GLX_F64, m, n, l, int(np.diff(ptr).max()), float(gw.min()), float(gcn.max()), csq, bn)
    s0, gap_p, rho = k.group_screen_guard_sw(rec, *args)
    if forced is not None:
        primal = 0.5 * rec[0] + mu * rec[2]
        rec[2] = (forced * primal - (0.5 * (1.0 + s0 * s0) * rec[0] + s0 * rec[1])) / mu
        s, gap_p, rho = k.group_screen_guard_sw(rec, *args)
        assert s == s0 and rho > 0.0 and gap_p > 0.0
    scr = ~gr.keep_mask(c["group_norms"], gcn, s0, rho, mu)
    assert not np.any(scr & nz)
    if forced is None:
        assert scr.sum() > 0


# ------------------------------------------------------------------------------------------ references
def test_the_two_numpy_references_agree_on_mask_and_integer_weights():
    """The reduction (sqrt(w) o A, sqrt(w) o b) against the row-subset and the row-duplicated problems:
    the weighted objective of either solution equals the other's to 1e-14 relative, in longdouble."""
    m, n, l, ratio = 40, 130, 3, 0.1
    for kind in ("mask", "int"):
        ref = sw.reference_solution(m, n, l, ratio, kind)
        A, b, w, mu = ref["A"], ref["b"], ref["w"], ref["mu"]
        rows = np.repeat(np.arange(m), w.astype(np.int64))       # a mask keeps, an integer weight repeats
        A2, b2 = A[rows], b[rows]
        assert abs(float(sw.mu_max(A, b, w)) - float(sw.cref.mu_max(A2.astype(sw.LD), b2.astype(sw.LD)))) <= 1e-14 * mu
        x2, _ = sr.fista_screen(A2, b2, mu, tol=2e-14, maxit=400000)
        p1 = float(sw.primal(ref["x"], A, b, mu, w))
        p2 = float(sw.primal(x2, A, b, mu, w))
        q2 = float(sw.cref.certificate(x2.astype(sw.LD), A2.astype(sw.LD), b2.astype(sw.LD), sw.LD(mu))["primal"])
        assert abs(p2 - q2) <= 1e-14 * p1            # the same function of x, two ways
        assert abs(p1 - p2) <= 1e-12 * p1            # two solves to the gap's floor (rel_gap <= 1e-12 each)


def test_cv_reference_indices():
    """The reference curve of the issue's instance (tests/test_gpu_sample_weight.py asserts these
    indices of the GPU's curve): best = 5, one_se = 4, at 1e-6."""
    A, b = sw.cv_instance()
    mus, fl = sw.cv_reference(A, b, tol=1e-6)
    mean, se, best, one = sw.cv_aggregate(fl)
    assert (best, one) == (5, 4)
    order = np.sort(mean)
    assert order[1] / order[0] - 1.0 > 0.01                      # the runner-up is more than 1 % away
    thr = mean[best] + se[best]
    assert mean[4] < thr * 0.99 and mean[3] > thr * 1.10         # the 1-SE threshold separates 3 and 4
