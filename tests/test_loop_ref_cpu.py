"""tests/loop_ref.py, the NumPy model of the certified solve's loop, held to what is already trusted,
and the facts of its cases that tests/test_gpu_certified_loop.py relies on. No GPU.

1. Run to tol = 2e-14 the model reaches screen_ref.reference_solution's objective within the two
   gaps, rows, groups and sample weights alike, and screens no row that is active there.
2. The histories of the cases the GPU test compares, as this model gives them (the GPU loop takes a
   compaction at its final check too, and so does the model), and min_margin >= 1e-6 in each: no
   screening decision sits within 1e-6 of its threshold, so the GPU's float64 roundings (~1e-15)
   cannot flip one and the GPU test compares decisions with no exemptions. Measured: >= 6.2e-5.
3. The model's own rules on a few small facts: maxit = 0, the final check, the 0.9 rule, the restart.
"""
import numpy as np
import pytest

import group_ref as gr
import loop_ref as lr
import screen_ref as sr
import sw_ref as sw

LD = np.longdouble


# ------------------------------------------------------------------------------------------ 1
def _primal_gap(p, x):
    if p["ptr"] is not None:
        c = gr.certificate(x.astype(LD), p["A"].astype(LD), p["b"].astype(LD), LD(p["mu"]), p["ptr"], p["gw"])
    elif p["w"] is not None:
        c = sw.certificate(x, p["A"], p["b"], p["mu"], p["w"])
    else:
        c = sr.cref.certificate(x.astype(LD), p["A"].astype(LD), p["b"].astype(LD), LD(p["mu"]))
    return c["primal"], c["gap"]


def test_converged_model_meets_the_reference_rows():
    m, n, l, ratio = 40, 130, 3, 0.1
    ref = sr.reference_solution(lr.SEED, m, n, l, ratio)
    x, info = lr.model(("rows", m, n, l, ratio), "f64", 400000, tol=2e-14)
    p = lr.problem("rows", m, n, l, ratio)
    assert p["mu"] == ref["mu"] and np.array_equal(p["A"], ref["A"])
    P, gap = _primal_gap(p, x)
    print("\nrows: %d iterations, %d rounds, history %s, rel_gap %.2e; |P - P_ref| %.2e, gaps %.2e + %.2e"
          % (info["iterations"], info["rounds"], info["kept_history"], info["rel_gap"], abs(float(P - ref["primal"])),
             float(gap), float(ref["gap"])))
    assert info["converged"] and info["rel_gap"] <= 2e-14
    assert abs(P - ref["primal"]) <= gap + ref["gap"]
    screened = np.ones(n, dtype=bool)
    screened[info["kept_rows"]] = False
    assert info["compactions"] >= 1 and screened.any()
    assert not np.any(screened & ~(ref["gtheta"] < LD(ref["mu"])))
    assert np.all(x[screened] == 0)


def test_converged_model_meets_the_reference_groups():
    m, n, l, pool, ratio = gr.CASES[4]
    ref = gr.reference_solution(m, n, l, pool, ratio)
    key = ("grp", m, n, l, ratio, False, pool)
    x, info = lr.model(key, "f64", 400000, tol=2e-14)
    P, gap = _primal_gap(lr.problem(*key), x)
    assert info["converged"]
    assert abs(P - ref["primal"]) <= gap + ref["gap"]
    screened = np.ones(ref["w"].size, dtype=bool)
    screened[info["kept_groups"]] = False
    assert not np.any(screened & ~(ref["gtheta"] < LD(ref["mu"])))
    assert np.array_equal(info["kept_rows"], np.nonzero(gr.expand_rows(~screened, ref["ptr"]))[0])


def test_converged_model_meets_the_reference_sample_weights():
    m, n, l, ratio = 40, 130, 3, 0.1
    ref = sw.reference_solution(m, n, l, ratio, "general")
    key = ("sw", m, n, l, ratio)
    x, info = lr.model(key, "f64", 400000, tol=2e-14)
    p = lr.problem(*key)
    assert abs(p["mu"] - ref["mu"]) <= 4 * sr.EPS64 * ref["mu"] and np.array_equal(p["w"], ref["w"])
    P, gap = _primal_gap(p, x)
    assert info["converged"]
    assert abs(P - ref["primal"]) <= gap + ref["gap"] + 16 * sr.EPS64 * abs(ref["primal"])   # (mu's last bits)
    screened = np.ones(n, dtype=bool)
    screened[info["kept_rows"]] = False
    assert not np.any(screened & ~(ref["gtheta"] < LD(ref["mu"])))


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("case", lr.LOOP_CASES + lr.BRANCH_CASES, ids=lambda c: c[0])
def test_histories_and_margins(case):
    name, key, maxit, check_every, x0_scale, want = case
    x, info = lr.model(key, "ld", maxit, check_every, True, x0_scale)
    x64, i64 = lr.model(key, "f64", maxit, check_every, True, x0_scale)
    print("\n%s: history %s, width %d, kept %d, checks %d, iterations %d, min_margin %.2e"
          % (name, info["kept_history"], info["width"], info["kept"], info["checks"], info["iterations"],
             info["min_margin"]))
    assert info["kept_history"] == want
    assert info["min_margin"] >= 1e-6 and i64["min_margin"] >= 1e-6
    for k in ("kept_history", "compactions", "width", "kept", "checks", "rounds", "iterations"):
        assert info[k] == i64[k], k                      # the float64 run decides as the longdouble one does
    assert np.array_equal(info["kept_rows"], i64["kept_rows"])
    assert info["rounds"] == 1 and not info["converged"] or want[-1:] == [0]
    off = np.ones(x.shape[0], dtype=bool)
    off[info["kept_rows"]] = False
    assert np.all(x[off] == 0)


def test_added_cases_compact_at_least_twice_by_45():
    for name in ("groups", "sample weights"):
        case = next(c for c in lr.LOOP_CASES if c[0] == name)
        assert case[2] == 45 and len(case[5]) >= 2


def test_the_kept_zero_cases_leave_a_nonzero_iterate():
    """A history that ends in 0 is written by the kept == 0 branch alone, which the loop reaches only
    where the stop rule is not met: the iterate it leaves is not yet zero (at x = 0 the gap is exactly
    0 here). Without screening the same solve iterates until x = 0, in another number of iterations."""
    for case in lr.BRANCH_CASES:
        name, key, maxit, check_every, x0_scale, want = case
        if want[-1:] != [0]:
            continue
        x, info = lr.model(key, "ld", maxit, check_every, True, x0_scale)
        xu, iu = lr.model(key, "ld", maxit, check_every, False, x0_scale)
        assert np.all(x == 0) and info["kept"] == 0 and info["kept_rows"].size == 0 and info["converged"]
        assert info["width"] == 0 and info["iterations"] < maxit and info["rel_gap"] == 0.0
        assert np.all(xu == 0) and iu["converged"] and iu["iterations"] != info["iterations"]


# ------------------------------------------------------------------------------------------ 3
def test_rules():
    key = ("rows", 40, 200, 3, 0.3)
    p = lr.problem(*key)
    x0 = lr.start(200, 3, 1.0)
    # maxit = 0: one check, x0 returned as it is
    x, info = lr.run(p["A"], p["b"], p["mu"], x0, 0, 10, True, np.float64)
    assert np.array_equal(x, x0) and info["iterations"] == 0 and info["checks"] == 1 and info["compactions"] == 0
    # a check after every check_every-th iteration and after the last
    for ce, K, checks in ((10, 45, 6), (3, 20, 8), (1, 20, 21), (7, 20, 4), (25, 20, 2), (10, 20, 3)):
        assert lr.model(key, "f64", K, ce)[1]["checks"] == checks
    # screening off: no decision, the iterates of a longer run are those of a shorter one
    xs, i_s = lr.model(key, "f64", 10, 10, False, None, (3,))
    assert i_s["compactions"] == 0 and i_s["width"] == 200 and np.array_equal(i_s["kept_rows"], np.arange(200))
    assert np.array_equal(i_s["snapshots"][3], lr.model(key, "f64", 3, 10, False)[0])
    # the 0.9 rule: a compaction's padded width is at most 0.9 of the width before it
    _, info = lr.model(key, "f64", 45, 10)
    widths = [200] + [lr.pad64(k) for k in info["kept_history"]]
    assert all(b * 10 <= a * 9 for a, b in zip(widths, widths[1:])) and info["width"] == widths[-1]
    # the restart: the iterate after a compaction is a plain proximal-gradient step from x (y = x)
    K = next(k for k in (10, 20, 30, 40) if lr.model(key, "f64", k, 10)[1]["compactions"] == 1)
    _, i10 = lr.model(key, "f64", K, 10)
    x10, _ = lr.model(key, "f64", K, 10, False)           # (the same iterates: the first compaction is at K)
    x11, i11 = lr.model(key, "f64", K + 1, 10)
    assert i11["kept_history"] == i10["kept_history"]
    rows = i10["kept_rows"]
    Ar = p["A"][:, rows]
    t = lr.step(p["A"])
    want = sr.prox(x10[rows] - t * (Ar.T @ (Ar @ x10[rows] - p["b"])), t * p["mu"])
    assert np.max(np.abs(x11[rows] - want)) <= 64 * sr.EPS64 * np.max(np.abs(want))
