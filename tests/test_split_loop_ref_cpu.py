"""CPU-only checks of tests/split_loop_ref.py, the loop model of the three splitting solvers.

* Run in float64 with NumPy's own setup it reproduces every admm_dual_*, admm_primal_* (both forms
  where Woodbury serves) and alm_dual_* golden to the figures tests/test_admm_cpu.py,
  tests/test_admm_primal_cpu.py and tests/test_alm_dual_cpu.py assert of the restatements.
* The stop-rule cases of split_loop_ref.STOP_CASES: with converge_len = 3 the streak becomes positive,
  resets, and later reaches 3 at the pinned k; every r_norm and s_norm stays the pinned margin
  (at least 1e-3) from thres, and the float64 and longdouble models' norms agree within 1e-9, so
  no decision of the stop rule is a tie.
* `splits` changes the last bits only, and the K = 1, 2, 3 snapshots are the iterates of shorter runs.
"""
import numpy as np
import pytest

import admm_primal_ref
import admm_ref
import alm_dual_ref
import split_loop_ref as sl
import test_admm_cpu
import test_admm_primal_cpu
import test_alm_dual_cpu


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - want) / np.abs(want)))


@pytest.mark.parametrize("name", test_admm_cpu.CASES)
def test_dual_admm_reproduces_golden(name):
    meta, arrs, A, b, x0, mu = test_admm_cpu.load_case(name)
    out = sl.dual_admm(x0, A, b, mu, admm_ref.inverse_factor(A, 1e2))
    assert out["k"] == int(arrs["k"])
    assert _rel(out["f_hist"], arrs["f_hist"]) <= 1e-10
    assert _rel(out["f_hist_best"], arrs["f_hist_best"]) <= 1e-10
    assert np.max(np.abs(out["x"] - arrs["x"])) <= 1e-10 * np.max(np.abs(arrs["x"]))
    assert np.allclose(out["r_norm"], arrs["r_norm"], rtol=1e-6, atol=0)
    assert np.allclose(out["s_norm"], arrs["s_norm"], rtol=1e-6, atol=1e-14)


@pytest.mark.parametrize("name,form", [(c, 1) for c in test_admm_primal_cpu.CASES]
                         + [(c, 2) for c in test_admm_primal_cpu.WIDE])
def test_primal_admm_reproduces_golden(name, form):
    meta, arrs, A, b, x0, mu = test_admm_primal_cpu.load_case(name)
    opts = dict(meta["opts"])
    rho = opts.get("rho", sl.PRIMAL_DEFAULTS["rho"])
    out = sl.primal_admm(x0, A, b, mu, *admm_primal_ref.setup(A, b, rho, form), form, opts=opts)
    assert out["k"] == int(arrs["k"])
    assert _rel(out["f_hist"], arrs["f_hist"]) <= 1e-8
    assert _rel(out["f_hist_best"], arrs["f_hist_best"]) <= 1e-8
    assert abs(out["fval"] - arrs["fval"]) <= 1e-8 * abs(arrs["fval"])
    assert np.max(np.abs(out["x"] - arrs["x"])) <= 1e-8 * np.max(np.abs(arrs["x"]))
    assert _rel(out["r_norm"], arrs["r_norm"]) <= 5e-6
    assert _rel(out["s_norm"], arrs["s_norm"]) <= 5e-6


@pytest.mark.parametrize("name", test_alm_dual_cpu.CASES)
def test_dual_alm_reproduces_golden(name):
    meta, arrs, A, b, x0, mu = test_alm_dual_cpu.load_case(name)
    opts = dict(meta["opts"])
    K = alm_dual_ref.inverse_factor(A, opts.get("rho", 1e2))
    out = sl.dual_alm(x0, A, b, mu, K, alm_dual_ref.inner_matrix(A, K, opts.get("rho", 1e2)), opts=opts)
    assert out["k"] == int(arrs["k"])
    bar = min(1e-9, max(1e-12, 50 * meta["restated_deviation"]["f_hist"]))
    assert _rel(out["f_hist"], arrs["f_hist"]) <= bar
    assert _rel(out["f_hist_best"], arrs["f_hist_best"]) <= bar
    assert abs(out["fval"] - arrs["fval"]) <= bar * abs(arrs["fval"])
    assert np.max(np.abs(out["x"] - arrs["x"])) <= 1e-9 * np.max(np.abs(arrs["x"]))
    assert _rel(out["r_norm"], arrs["r_norm"]) <= 3e-5
    assert _rel(out["s_norm"], arrs["s_norm"]) <= 3e-5


def _stop_run(case, dtype):
    solver, shape, form, extra, thres, k, margin = case
    A, b, x0, mu = sl.instance(*shape)
    rho = extra.get("rho", sl.PRIMAL_DEFAULTS["rho"] if solver == "primal" else 1e2)
    mats = sl.numpy_setup(solver, A, b, rho, form)
    return sl.run(solver, shape, mats, {**extra, "thres": thres, "converge_len": 3, "maxit": 60}, dtype)


@pytest.mark.parametrize("case", sl.STOP_CASES, ids=["%s-%dx%dx%d-form%d" % ((c[0],) + c[1] + (c[2],))
                                                      for c in sl.STOP_CASES])
def test_stop_cases_pass_through_a_reset(case):
    solver, shape, form, extra, thres, k, margin = case
    r = _stop_run(case, "f64")
    L = r["length"]
    assert r["k"] == k and len(r["f_hist"]) == k and L[-1] == 3
    first = int(np.argmax(L > 0))
    assert L[first] > 0 and np.any(L[first + 1:k - 3] == 0), L   # positive, reset, then the final streak
    norms = np.concatenate([r["r_norm"], r["s_norm"]])
    got = float(np.min(np.abs(norms / thres - 1)))
    print(solver, shape, form, "k", k, "margin %.4g" % got, "streak", L.tolist())
    assert got >= margin >= 1e-3
    ld = _stop_run(case, "ld")
    assert ld["k"] == k and np.array_equal(ld["length"], L)
    assert _rel(r["r_norm"], ld["r_norm"]) <= 1e-9 and _rel(r["s_norm"], ld["s_norm"]) <= 1e-9


def test_splits_and_snapshots():
    shape = (100, 130, 3)
    A, b, x0, mu = sl.instance(*shape)
    for solver, opts in (("dual", {}), ("primal", {}), ("alm", {"inner_iters": 7})):
        mats = sl.numpy_setup(solver, A, b, sl.PRIMAL_DEFAULTS["rho"] if solver == "primal" else 1e2, 1)
        o = {**opts, "thres": 0.0, "maxit": 3}
        full = sl.run(solver, shape, mats, o, "f64", snap=(1, 2, 3))
        assert full["k"] == 3 and np.array_equal(full["snapshots"][3], full["x"])
        for K in (1, 2):
            short = sl.run(solver, shape, mats, {**o, "maxit": K}, "f64")
            assert np.array_equal(short["x"], full["snapshots"][K])
            assert np.array_equal(short["f_hist"], full["f_hist"][:K])
        for S in (2, 3):
            sp = sl.run(solver, shape, mats, o, "f64", splits=S)
            d = np.max(np.abs(sp["x"] - full["x"])) / np.max(np.abs(full["x"]))
            assert 0 < d <= 1e-9, (solver, S, d)
        zero = sl.run(solver, shape, mats, {**o, "maxit": 0}, "f64")
        assert zero["k"] == 0 and np.array_equal(zero["x"], x0) and len(zero["f_hist"]) == 0
        f0 = 0.5 * np.sum((A @ x0 - b) ** 2) + mu * np.sum(np.linalg.norm(x0, axis=1))
        assert abs(zero["fval"] - f0) <= 1e-12 * f0
        assert sl.run(solver, shape, mats, {**o, "maxit": 9, "max_total_iters": 2}, "f64")["k"] == 2
    M, X = np.arange(12.0).reshape(3, 4), np.arange(8.0).reshape(4, 2)
    for S in (1, 2, 3, 4):
        assert np.array_equal(sl.mm(M, X, S), M @ X)


def test_alm_objective_rises_with_one_inner_step():
    """The arm tests/test_gpu_split_loops.py uses to see f_hist_best leave f_hist: (100, 130, 3) with
    one inner step rises at iterations 25, 27 and 29, each by more than 5e-7 relative."""
    shape = (100, 130, 3)
    A, b, x0, mu = sl.instance(*shape)
    r = sl.run("alm", shape, sl.numpy_setup("alm", A, b, 1e2), {"thres": 0.0, "maxit": 30, "inner_iters": 1}, "f64")
    f = r["f_hist"]
    rises = np.nonzero(np.diff(f) > 0)[0] + 2
    assert list(rises) == [25, 27, 29]
    assert np.all(np.diff(f)[rises - 2] >= 5e-7 * f[rises - 1])
    assert np.all(r["f_hist_best"][rises - 1] < f[rises - 1])
