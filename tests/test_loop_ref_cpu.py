"""tests/loop_ref.py, the NumPy model of the certified solve's loop, held to what is already trusted,
and the facts of its cases that tests/test_gpu_certified_loop.py relies on. No GPU.

1. Run to tol = 2e-14 the model reaches screen_ref.reference_solution's objective within the two
   gaps, rows, groups and sample weights alike, and screens no row that is active there. The same for
   the intercept arm against ic_ref.reference_solution (weights, and none) and
   ic_ref.group_reference_solution, and for the sparse-group arm against sgl_ref.reference_solution
   (tau = 0.3 and 1): no row and no group of the reference's support is screened.
2. The histories of the cases the GPU test compares, as this model gives them (the GPU loop takes a
   compaction at its final check too, and so does the model), and min_margin >= 1e-6 in each: no
   screening decision sits within 1e-6 of its threshold, so the GPU's float64 roundings (~1e-15)
   cannot flip one and the GPU test compares decisions with no exemptions. Measured: >= 6.2e-5.
   The intercept and sparse-group cases pin kept_history too, the latter kept_row_history beside it
   (loop_ref.ROW_HISTORIES); their margins cover both sparse-group tests, and with them the 56
   halvings of k_sgl_dual_scale, which leave s within (1 + (1 - tau) w_g / tau) 2^-56 relative.
   Measured min_margin: ic weights 1.3e-4, ic 5.3e-4, ic ce=3 1.2e-3, ic groups 5.1e-4; sgl tau=0.3
   8.5e-4 (l=16: 9.0e-4), tau=0.9 long 4.0e-4, tau=1 5.5e-5, weights 3.4e-3, ce=3 1.1e-3; kept=0: ic
   3.0e-2 (ce=1: 1.8e-3), sgl 3.2e-3. What each case is there for is asserted as a fact of the model.
3. The model's own rules on a few small facts: maxit = 0, the final check, the 0.9 rule, the restart.
"""
import numpy as np
import pytest

import group_ref as gr
import ic_ref as ic
import loop_ref as lr
import screen_ref as sr
import sgl_ref as sg
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


def _assert_meets(name, x, info, P, gap, ref, slack=0.0):
    print("\n%s: %d iterations, %d rounds, history %s, rel_gap %.2e; |P - P_ref| %.2e, gaps %.2e + %.2e"
          % (name, info["iterations"], info["rounds"], info["kept_history"], info["rel_gap"],
             abs(float(P - ref["primal"])), float(gap), float(ref["gap"])))
    assert info["converged"] and info["rel_gap"] <= 2e-14
    assert abs(P - ref["primal"]) <= gap + ref["gap"] + slack


@pytest.mark.parametrize("kind", ["general", "ones"])
def test_converged_model_meets_the_reference_intercept(kind):
    """The intercept arm against ic_ref.reference_solution (the centred pair's fixed point): with sample
    weights, and with none (the model's weights of one and sigma = m; the reference's are "ones")."""
    m, n, l, ratio = 40, 130, 3, 0.1
    ref = ic.reference_solution(m, n, l, ratio, kind)
    key = ("ic", m, n, l, ratio, False, None, None, "general") if kind == "general" else ("ic", m, n, l, ratio)
    p = lr.problem(*key)
    assert p["mu"] == ref["mu"] and np.array_equal(p["A"], ref["A"]) and p["ic"]
    assert np.array_equal(p["w"], ref["w"]) if kind == "general" else p["w"] is None
    x, info = lr.model(key, "f64", 400000, tol=2e-14)
    c = ic.certificate(x, p["A"], p["b"], p["mu"], ref["w"])
    _assert_meets("intercept, " + kind, x, info, c["primal"], c["gap"], ref)
    screened = np.ones(n, dtype=bool)
    screened[info["kept_rows"]] = False
    assert info["compactions"] >= 1 and screened.any()
    assert not np.any(screened & ~(ref["gtheta"] < LD(ref["mu"])))
    assert np.all(x[screened] == 0)
    # the intercept the model reports is the returned x's, and the reference's within what x's distance allows
    assert np.array_equal(info["intercept"], ic.intercept_of(x, p["A"], p["b"], ref["w"]))
    am = np.max(np.abs(ic.col_means(p["A"], ref["w"])))
    assert np.max(np.abs(info["intercept"] - ref["c"])) <= am * np.sum(np.abs(x.astype(LD) - ref["x"]))


def test_converged_model_meets_the_reference_intercept_groups():
    m, n, l, ratio = 40, 130, 3, 0.5      # (at 0.1 the kept groups never fit 64 columns: no compaction)
    ref = ic.group_reference_solution(m, n, l, ratio)
    key = ("icg", m, n, l, ratio, False, None, None, "general")
    p = lr.problem(*key)
    assert p["mu"] == ref["mu"] and np.array_equal(p["ptr"], ref["ptr"]) and np.array_equal(p["gw"], ref["gw"])
    x, info = lr.model(key, "f64", 400000, tol=2e-14)
    c = ic.certificate(x, p["A"], p["b"], p["mu"], p["w"], p["ptr"], p["gw"])
    _assert_meets("intercept, groups", x, info, c["primal"], c["gap"], ref)
    screened = np.ones(ref["gw"].size, dtype=bool)
    screened[info["kept_groups"]] = False
    assert info["compactions"] >= 1 and screened.any()
    assert not np.any(screened & ~(ref["gtheta"] < LD(ref["mu"])))
    assert np.array_equal(info["kept_rows"], np.nonzero(gr.expand_rows(~screened, ref["ptr"]))[0])


@pytest.mark.parametrize("case", [sg.CASES[2], sg.CASES[3]], ids=lambda c: "%dx%dx%d-tau=%g" % (c[0], c[1], c[2], c[4]))
def test_converged_model_meets_the_reference_sparse_group(case):
    m, n, l, pool, tau, ratio = case
    ref = sg.reference_solution(m, n, l, pool, tau, ratio)
    key = ("sgl", m, n, l, ratio, False, pool, tau)
    p = lr.problem(*key)
    assert p["mu"] == ref["mu"] and p["tau"] == tau and np.array_equal(p["ptr"], ref["ptr"])
    x, info = lr.model(key, "f64", 400000, tol=2e-14)
    c = sg.certificate(x.astype(LD), p["A"].astype(LD), p["b"].astype(LD), LD(p["mu"]), p["ptr"], p["gw"], tau)
    _assert_meets("sparse-group, tau = %g" % tau, x, info, c["primal"], c["gap"], ref)
    screened = np.ones(n, dtype=bool)
    screened[info["kept_rows"]] = False
    assert info["compactions"] >= 1 and screened.any()
    assert not np.any(screened & ref["support"])                     # no row of the support is screened,
    gone = np.ones(ref["w"].size, dtype=bool)
    gone[info["kept_groups"]] = False
    assert not np.any(gr.expand_rows(gone, ref["ptr"]) & ref["support"])   # and no group that holds one
    assert np.all(x[screened] == 0)
    assert len(info["kept_row_history"]) == len(info["kept_history"]) == info["compactions"]


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
    assert (key[0] == "sgl") == (name in lr.ROW_HISTORIES) == ("kept_row_history" in info)
    if key[0] == "sgl":     # the rows beside the groups: pinned, the float64 run's too, never fewer than the groups
        print("    rows %s (of the surviving groups: %s)" % (info["kept_row_history"], info["group_row_history"]))
        assert info["kept_row_history"] == lr.ROW_HISTORIES[name] == i64["kept_row_history"]
        assert all(r >= g for r, g in zip(info["kept_row_history"], info["kept_history"]))
        assert np.array_equal(info["kept_groups"], i64["kept_groups"])
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


def _case(name):
    return next(c for c in lr.LOOP_CASES + lr.BRANCH_CASES if c[0] == name)


def test_the_intercept_and_sparse_group_cases_are_what_the_gpu_test_needs():
    """What each added case is there for, as facts of the model (the histories themselves are pinned above)."""
    for name, least in (("ic weights", 2), ("ic", 1), ("ic groups", 2), ("sgl tau=0.3", 2), ("sgl tau=0.9 long", 1),
                        ("sgl tau=1", 1), ("sgl weights", 1)):
        c = _case(name)
        assert c[2] == 45 and c[3] == 10 and len(c[5]) >= least, name
    assert lr.problem(*_case("ic weights")[1])["w"] is not None and lr.problem(*_case("ic")[1])["w"] is None
    assert lr.problem(*_case("sgl weights")[1])["w"] is not None
    for name in ("ic ce=3", "sgl ce=3"):
        assert _case(name)[3] == 3 and len(_case(name)[5]) >= 1
    # tau = 0.3, short groups: a compaction that removes interior rows of a group that survives (fewer rows
    # kept than the kept groups hold) and one that drops whole groups
    name, key, maxit, ce, x0s, want = _case("sgl tau=0.3")
    p = lr.problem(*key)
    _, info = lr.model(key, "ld", maxit, ce, True, x0s)
    assert int(np.diff(p["ptr"]).max()) <= 8 and p["tau"] == 0.3
    assert any(r < g for r, g in zip(info["kept_row_history"], info["group_row_history"]))
    groups = [p["gw"].size] + info["kept_history"]
    assert any(b < a for a, b in zip(groups, groups[1:]))
    # tau = 0.9: a run longer than the 64 lanes of a wave cover in one trip; tau = 1: the group test is off
    p = lr.problem(*_case("sgl tau=0.9 long")[1])
    assert p["tau"] == 0.9 and int(np.diff(p["ptr"]).max()) == 65
    assert lr.problem(*_case("sgl tau=1")[1])["tau"] == 1.0
    # the kept == 0 branches: mu = 1.05 mu_max from start(n, l, 1.0)
    for name in ("ic kept=0", "ic kept=0-ce=1", "sgl kept=0"):
        c = _case(name)
        assert c[1][4] == 1.05 and c[4] == 1.0 and c[5][-1] == 0


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
